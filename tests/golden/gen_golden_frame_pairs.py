"""Generate tests/golden/g35_frame_pairs.npz by running the reference's own BaseDataset.compute_crop_params and
BaseDataset.flow_process (dataloader/vidbase.py, with ext_utils/flowlib.warp_flow) on the CPU (development container only, like
gen_golden_cse.py).  OpenCV is not installed, so a module named `cv2` is installed first whose `remap` is the restatement in
tests/framepair_numpy.py: the record pins everything EXCEPT the sampler itself to a reference run -- the integer box arithmetic,
int(1.2 * length), the np.dot that forms hp0, np.linalg.inv of the crop matrices, the fp32 storage of the re-expressed flows, the
map formed by warp_flow, the norm, the exponential, the threshold and the NDC scaling.  Inputs and outputs only.

Keys: `names`, and per case `<name>/masks` (2,h,w) uint8, `<name>/img_size`, `<name>/flow_c` (2,2,S,S) fp32 (the cropped flows of
the pair, made by the oracle's crop of `<name>/flow_raw` (2,h,w,2)), with the reference's `<name>/kaug` (2,4) float64,
`<name>/x0`, `<name>/y0` (2,S,S) fp32 (hp0 as read_raw casts it), `<name>/flow` (2,2,S,S) fp32 and `<name>/occ` (2,S,S) float64.

The fixtures' own precondition is asserted here: on every case the oracle's exemptions cover at most 1 % of a plane.

    python tests/golden/gen_golden_frame_pairs.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import framepair_numpy as O  # noqa: E402

CASES = (("s16", 24, 40, 16, 3), ("s32", 37, 65, 32, 4), ("s24", 37, 65, 24, 5))     # name, h, w, img_size, seed


def _cv2_remap(src, map1, map2=None, interpolation=1, **kw):
    """cv2.remap through the oracle's sampler: src (H,W) | (H,W,C); float maps (H,W) x 2 or one (H,W,2)."""
    src = np.asarray(src)
    if map2 is None:
        map1, map2 = map1[..., 0], map1[..., 1]
    planes = src[..., None] if src.ndim == 2 else src
    out = []
    for c in range(planes.shape[-1]):
        if interpolation == 0:
            out.append(O.sample_nearest(planes[..., c], map1, map2)[0][0])
        else:
            out.append(O.sample_linear(planes[..., c], map1, map2)[0])
    out = np.stack(out, -1).astype(src.dtype)
    return out[..., 0] if src.ndim == 2 else out


def install_cv2():
    cv2 = types.ModuleType("cv2")
    cv2.remap, cv2.INTER_NEAREST, cv2.INTER_LINEAR = _cv2_remap, 0, 1
    sys.modules["cv2"] = cv2
    absl = types.ModuleType("absl")
    absl.flags, absl.app = types.ModuleType("absl.flags"), types.ModuleType("absl.app")
    sys.modules.update({"absl": absl, "absl.flags": absl.flags, "absl.app": absl.app})


def blob_mask(rng, h, w):
    yy, xx = np.mgrid[:h, :w]
    cy, cx = rng.uniform(0.35, 0.65) * h, rng.uniform(0.35, 0.65) * w
    ry, rx = rng.uniform(0.2, 0.33) * h, rng.uniform(0.2, 0.33) * w
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) < 1).astype(np.uint8)


def pair_flows(rng, h, w):
    """A forward flow and a roughly inverse backward flow, (2,h,w,2) fp32: partly consistent, partly not."""
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    d = np.stack([1.5 + 0.8 * np.sin(yy / 5.0), -1.0 + 0.6 * np.cos(xx / 7.0)], -1)
    noise = rng.standard_normal((h, w, 2)) * 0.15 * (rng.random((h, w, 1)) < 0.7)
    return np.stack([d + rng.standard_normal((h, w, 2)) * 0.05, -d + noise]).astype(np.float32)


def main():
    install_cv2()
    _ref_import.install_stubs()
    for p in (_ref_import.REF + "/nnutils", _ref_import.REF + "/third_party", _ref_import.REF):
        sys.path.insert(0, p)
    from dataloader.vidbase import BaseDataset
    out = {"names": np.asarray([c[0] for c in CASES])}
    for name, h, w, S, seed in CASES:
        rng = np.random.default_rng(seed)
        ds = BaseDataset({"img_size": S})
        masks = np.stack([blob_mask(rng, h, w), blob_mask(rng, h, w)])
        raw = pair_flows(rng, h, w)
        got = [ds.compute_crop_params(m[..., None].astype(np.float64)) for m in masks]      # kaug, hp0, A, B
        box, _ = O.mask_bbox(masks)
        (_, aff, status), _ = O.compute_crop_params(box, S)
        assert status.sum() == 0
        crop, _ = O.crop_frames(aff, S, flow=raw)
        flow_c = crop["flow"].astype(np.float32)
        fl = [np.ascontiguousarray(flow_c[k].transpose(1, 2, 0)).copy() for k in range(2)]
        zeros = np.zeros((S, S), np.float32)
        flow, flown, occ, occn = ds.flow_process(fl[0], fl[1], zeros, zeros, got[0][1], got[1][1], got[0][2], got[0][3], got[1][2],
                                                 got[1][3])
        _, _, exempt = O.flow_process(flow_c, aff, S)
        assert exempt.reshape(2, -1).mean(1).max() <= 0.01, (name, exempt.reshape(2, -1).mean(1))
        out.update({f"{name}/masks": masks, f"{name}/img_size": np.int64(S), f"{name}/flow_raw": raw, f"{name}/flow_c": flow_c,
                    f"{name}/kaug": np.stack([g[0] for g in got]),
                    f"{name}/x0": np.stack([g[1][:, :, 0].astype(np.float32) for g in got]),
                    f"{name}/y0": np.stack([g[1][:, :, 1].astype(np.float32) for g in got]),
                    f"{name}/flow": np.stack([flow, flown]).astype(np.float32), f"{name}/occ": np.stack([occ, occn])})
    path = os.path.join(HERE, "g35_frame_pairs.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
