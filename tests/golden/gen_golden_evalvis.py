"""Generate tests/golden/g39_evalvis.npz by running the reference's own flow_to_image / make_color_wheel
(third_party/ext_utils/flowlib.py) and image_grid (nnutils/vis_utils.py) on the CPU (development container only, like
gen_golden_nvs.py; png and cv2 are stubbed by _ref_import.install_stubs()).  Inputs and outputs only.

Every flow case runs twice, on the fp32 array and on its float64 copy (copies: the reference zeroes unknown pixels in place).
With numpy >= 2 the fp32 run is float64 after `u / (maxrad + np.finfo(float).eps)`; the numpy version is recorded.

Keys: numpy_version, wheel (55,3); per flow case c in CASES: c/flow (H,W,2|3) fp32, c/img32, c/img64 (H,W,3) uint8, c/ndiff = the
count of channels where the two differ; grid/img (9,4,5,3) fp32, grid/out (12,15,3); grid1/img (3,2,2,1), grid1/out (2,2,1) for
image_grid(., 1, 1).  The eval() block and save_vid are methods of classes behind heavy imports: not run here.

    python tests/golden/gen_golden_evalvis.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402


def cases():
    rng = np.random.default_rng(39)
    out = {}
    out["rand64"] = (3.0 * rng.standard_normal((64, 64, 2))).astype(np.float32)
    yy, xx = np.mgrid[:64, :64].astype(np.float32)
    out["smooth64"] = np.stack([np.sin(xx / 9.0) * 4 + yy / 16.0, np.cos(yy / 7.0) * 3 - xx / 20.0], -1).astype(np.float32)
    f = (0.5 * rng.standard_normal((33, 31, 3))).astype(np.float32)               # a third channel, unknown flow
    f[0, 0, 0] = 1e8
    f[7, 9, 1] = -np.inf
    f[32, 30] = [2e7, -3e7, 0]
    out["unknown33x31"] = f
    f = rng.standard_normal((5, 7, 2)).astype(np.float32)                          # a NaN: the frame is normalised by -1
    f[2, 3, 0] = np.nan
    out["nan5x7"] = f
    out["zero5x7"] = np.zeros((5, 7, 2), np.float32)
    out["one1x1"] = np.asarray([[[0.3, -0.4]]], np.float32)
    return out


def main():
    _ref_import.install_stubs()
    sys.path.insert(0, os.path.join(_ref_import.REF, "third_party", "ext_utils"))
    sys.path.insert(0, os.path.join(_ref_import.REF, "nnutils"))
    import flowlib
    import vis_utils
    out = {"numpy_version": np.asarray(np.__version__), "wheel": flowlib.make_color_wheel()}
    for name, flow in cases().items():
        with np.errstate(all="ignore"):
            i32 = flowlib.flow_to_image(flow.copy())
            i64 = flowlib.flow_to_image(flow.astype(np.float64))
        out[name + "/flow"], out[name + "/img32"], out[name + "/img64"] = flow, i32, i64
        out[name + "/ndiff"] = np.int64((i32 != i64).sum())
        print(name, flow.shape, "channels that differ between the fp32 and the float64 run:", int(out[name + "/ndiff"]))
    rng = np.random.default_rng(40)
    img = rng.standard_normal((9, 4, 5, 3)).astype(np.float32)
    out["grid/img"], out["grid/out"] = img, vis_utils.image_grid(torch.from_numpy(img), 3, 3).numpy()
    img = rng.standard_normal((3, 2, 2, 1)).astype(np.float32)
    out["grid1/img"], out["grid1/out"] = img, vis_utils.image_grid(torch.from_numpy(img), 1, 1).numpy()
    path = os.path.join(HERE, "g39_evalvis.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
