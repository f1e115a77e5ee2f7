"""Generate tests/golden/g31_total_loss_bits.npz ON THE GPU, at the commit whose bits are to be pinned: the raw fp32 bits of
loss_utils.total_loss' total, of every weighted term and of every input gradient over the seeded inputs of
tests/lossasm_cases.total_loss_bits_case.  Only the public total_loss and .backward() are called; outputs only -- the test
(tests/test_gpu_lossasm.py::test_total_loss_reproduces_the_recorded_bits) rebuilds the inputs from the seed.

Recorded at the last commit where total_loss ran through a kernel pair of its own (ABI 9), so that the route through the one
loss assembly is held to that kernel's bits and not to its own.

To record again: check out that commit (the parent of the one that added this file), copy this file and tests/lossasm_cases.py
(which holds the seeded inputs and did not have them there) over it, build, and run on the GPU

    python tests/golden/gen_golden_total_loss_bits.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":                      # (the test that loads this module has tests/ and the package on its path already)
    sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import lossasm_cases as cases  # noqa: E402


def bits(t):
    return t.detach().cpu().numpy().astype(np.float32).view(np.uint32)


def run_case(N, wide, empty):
    """-> {name: uint32 bits} of one case: 'total', 'term_<name>', 'grad_<input key>'."""
    from moda_amd import loss_utils as LU
    rendered = {k: torch.as_tensor(v).to("cuda") for k, v in cases.total_loss_bits_case(N, wide, empty).items()}
    for k in cases.TOTAL_LOSS_BITS_INPUTS:
        rendered[k].requires_grad_(True)
    total, terms = LU.total_loss(rendered)
    total.backward()
    out = {"total": bits(total)}
    out.update({"term_" + n: bits(t) for n, t in terms.items()})
    out.update({"grad_" + k: bits(rendered[k].grad) for k in cases.TOTAL_LOSS_BITS_INPUTS})
    return out


def case_name(N, wide, empty):
    return f"n{N}" + ("_wide" if wide else "") + ("_empty" if empty else "")


def main():
    out = {}
    for case in cases.TOTAL_LOSS_BITS_CASES:
        out.update({f"{case_name(*case)}/{k}": v for k, v in run_case(*case).items()})
    path = os.path.join(HERE, "g31_total_loss_bits.npz")
    if len(sys.argv) > 1:
        path = sys.argv[1]
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
