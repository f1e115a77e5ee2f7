"""Writes tests/golden/g28_fscore.npz: the reference's own fscore (third_party/fscore.py, pure torch) on recorded squared
distances.  Needs the reference checkout that tests/golden/_ref_import.py names; only its outputs are stored.

  python tests/golden/gen_golden_pointset.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF  # noqa: E402

sys.path.insert(0, os.path.join(REF, "third_party"))
import fscore as ref_fscore  # noqa: E402


def main():
    rng = np.random.default_rng(28)
    out = {}
    cases = [
        ("a", rng.random((2, 301)) ** 2 * 4e-3, rng.random((2, 517)) ** 2 * 4e-3, [1e-3, 1e-4, 4e-3, 2.5e-7]),
        ("b", rng.random((1, 64)) * 1e-2 + 1e-3, rng.random((1, 33)) * 1e-2 + 1e-3, [1e-3, 5e-3, 1.0]),   # 1e-3: both precisions 0
        ("c", np.concatenate([rng.random((3, 40)) * 1e-3, np.zeros((3, 5))], 1), rng.random((3, 7)) + 1.0, [1e-3, 5e-4]),  # one side 0
    ]
    names = []
    for name, d1, d2, thrs in cases:
        d1, d2 = d1.astype(np.float32), d2.astype(np.float32)
        d1[0, :3] = np.float32(thrs[0])                     # values equal to a threshold: the comparison is strict
        out[f"{name}_dist1"], out[f"{name}_dist2"], out[f"{name}_thresholds"] = d1, d2, np.asarray(thrs, np.float64)
        res = [ref_fscore.fscore(torch.from_numpy(d1), torch.from_numpy(d2), threshold=t) for t in thrs]
        for k, key in enumerate(("fscore", "precision_1", "precision_2")):
            out[f"{name}_{key}"] = np.stack([r[k].numpy() for r in res])
        names.append(name)
    out["default_threshold_fscore"] = ref_fscore.fscore(torch.from_numpy(out["a_dist1"]), torch.from_numpy(out["a_dist2"]))[0].numpy()
    out["cases"] = np.asarray(names)
    assert (out["b_fscore"][0] == 0).all() and (out["b_precision_1"][0] == 0).all() and (out["b_precision_2"][0] == 0).all()
    np.savez_compressed(os.path.join(HERE, "g28_fscore.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
