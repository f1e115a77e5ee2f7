"""CPU: the oracle of the optimiser stage (tests/optim_numpy.py) against torch -- the float64 schedule against
torch.optim.lr_scheduler.OneCycleLR with the reference's arguments (nnutils/train_utils.py:261-290), the fp32 AdamW restatement
against torch.optim.AdamW in float64 -- and the host side of moda_amd.optim: group factors, the groups of the harness's names, the
tables, the bindings, the tensors it refuses.

The AdamW bar is measured, not chosen: torch's own fp32 CPU AdamW is run against torch's float64 AdamW on the same inputs, and the
restatement -- which differs from torch's fp32 run only in rounding order -- may be at most twice that far from float64.  Measured
here over the 14 steps of optim_numpy's case (largest absolute parameter difference over all tensors): torch fp32 2.25e-7, the
restatement 2.25e-7 (they agree to the last printed digit; the figures are printed by the test)."""
import os
import re

import numpy as np
import pytest
import torch

import optim_numpy as on
from moda_amd import _lib, optim as OP, train_utils as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = len(TU.GRAD_GROUPS)


# ---- schedule ---------------------------------------------------------------------------------------------------------------------
def torch_schedule(max_lr, total_steps, pct_start):
    """lr of every group at last_epoch 0..total_steps from torch itself: 22 groups, the reference's arguments."""
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in max_lr]
    opt = torch.optim.AdamW([{"params": [p]} for p in ps], lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-4)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, list(max_lr), total_steps, pct_start=pct_start, cycle_momentum=False,
                                              anneal_strategy="linear", final_div_factor=1. / 5, div_factor=25)
    rows = [[g["lr"] for g in opt.param_groups]]
    for _ in range(total_steps):
        opt.step()
        sch.step()
        rows.append([g["lr"] for g in opt.param_groups])
    with pytest.raises(ValueError):
        opt.step()
        sch.step()                                        # one more than total_steps: torch refuses
    return rows


@pytest.mark.parametrize("total_steps", [4, 40])
@pytest.mark.parametrize("num_epochs", [4, 10])
def test_schedule_is_torchs_one_cycle(total_steps, num_epochs):
    pct_start = 2. / num_epochs
    max_lr = [f * 5e-4 for f in OP.group_lr_factors("exp")]
    assert len(max_lr) == G
    rows = torch_schedule(max_lr, total_steps, pct_start)
    worst = 0.0
    for t, row in enumerate(rows):
        for mx, ref in zip(max_lr, row):
            got, past = on.one_cycle_lr(mx, total_steps, pct_start, t)
            assert not past
            worst = max(worst, abs(got - ref) / abs(ref))
    print(f"total_steps {total_steps}, num_epochs {num_epochs}: worst relative difference to torch {worst:.3g}")
    assert worst <= 1e-15
    # past total_steps the value is held and the overrun is told
    for t in (total_steps + 1, total_steps + 7):
        for mx, ref in zip(max_lr, rows[-1]):
            got, past = on.one_cycle_lr(mx, total_steps, pct_start, t)
            assert past and got == on.one_cycle_lr(mx, total_steps, pct_start, total_steps)[0] and abs(got - ref) <= 1e-15 * abs(ref)
    OP.check_schedule(total_steps, pct_start)


def test_schedule_of_the_shared_case_peaks_at_step_7():
    lr = [on.one_cycle_lr(1.0, on.TOTAL_STEPS, on.PCT_START, t)[0] for t in range(on.N_STEPS)]
    assert int(np.argmax(lr)) == 7 and lr[7] == 1.0 and lr[0] == 1.0 / 25 and lr[6] < lr[7] > lr[8]


def test_a_phase_of_no_length_is_refused():
    with pytest.raises(ValueError):
        OP.check_schedule(10, 0.1)                        # pct_start * total_steps - 1 == 0: torch divides 0 by 0 at step 0
    with pytest.raises(ValueError):
        OP.check_schedule(10, 1.0)                        # both phases end at total_steps - 1
    with pytest.raises(ValueError):
        OP.check_schedule(0, 0.2)
    with pytest.raises(ValueError):
        OP.check_schedule(10, 1.5)


# ---- AdamW ------------------------------------------------------------------------------------------------------------------------
def case_groups():
    return {n: TU.grad_group(n) for n, _, _, _ in on.TENSORS if TU.grad_group(n) is not None}


def case_max_lr():
    return [f * on.LEARNING_RATE for f in OP.group_lr_factors(on.ROOT_BASIS)]


def run_torch(dtype):
    """torch.optim.AdamW over 22 groups + OneCycleLR, the reference's construction, on the shared case."""
    params = {n: torch.nn.Parameter(torch.from_numpy(a).to(dtype)) for n, a in on.make_params().items()}
    groups = [[] for _ in range(G)]
    for n, g in case_groups().items():
        groups[g].append(params[n])
    opt = torch.optim.AdamW([{"params": g} for g in groups], lr=on.LEARNING_RATE, betas=(0.9, 0.999), weight_decay=1e-4)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, case_max_lr(), on.TOTAL_STEPS, pct_start=on.PCT_START, cycle_momentum=False,
                                              anneal_strategy="linear", final_div_factor=1. / 5, div_factor=25)
    for step in range(1, on.N_STEPS + 1):
        for n, g in on.make_grads(step).items():
            params[n].grad = None if g is None else torch.from_numpy(g).to(dtype)
        opt.step()
        sch.step()
    return {n: p.detach().double().numpy() for n, p in params.items()}


def run_oracle():
    groups = case_groups()
    o = on.Oracle({n: a for n, a in on.make_params().items() if n in groups}, groups, case_max_lr(), on.TOTAL_STEPS, on.PCT_START)
    for step in range(1, on.N_STEPS + 1):
        o.step({n: g for n, g in on.make_grads(step).items() if n in groups})
    return o


def test_adamw_restatement_against_torch_float64():
    ref, t32, o = run_torch(torch.float64), run_torch(torch.float32), run_oracle()
    d_torch = max(float(np.abs(t32[n] - ref[n]).max()) for n in o.p)
    d_ours = max(float(np.abs(o.p[n].astype(np.float64) - ref[n]).max()) for n in o.p)
    print(f"largest |parameter - float64 torch| after {on.N_STEPS} steps: torch fp32 {d_torch:.3g}, the restatement {d_ours:.3g}")
    assert d_torch > 0 and d_ours <= 2 * d_torch
    # the parameters moved by far more than that, every one of them: the bar is not met by standing still
    start = on.make_params()
    for n in o.p:
        assert float(np.abs(o.p[n] - start[n]).min()) > 0 and float(np.abs(ref[n] - start[n]).max()) > 100 * d_torch, n
    assert np.array_equal(ref["mystery.weight"], start["mystery.weight"].astype(np.float64))          # in no group: not optimised
    assert o.k["skin_aux"] == on.N_STEPS - 2 and o.k["bones"] == on.N_STEPS and o.t == on.N_STEPS and o.overrun == 0


def test_zero_gradient_still_moves_the_parameters():
    """After a rejected step the reference's gradients are zeros and AdamW still steps: decay and momentum move the parameters."""
    groups = case_groups()
    o = on.Oracle({n: a for n, a in on.make_params().items() if n in groups}, groups, case_max_lr(), on.TOTAL_STEPS, on.PCT_START)
    for step in range(1, 5):
        o.step({n: g for n, g in on.make_grads(step).items() if n in groups})
    before, k = o.p["bones"].copy(), o.k["bones"]
    g5 = on.make_grads(5)
    assert not g5["bones"].any()
    o.step({n: g for n, g in g5.items() if n in groups})
    assert o.k["bones"] == k + 1 and (o.p["bones"] != before).all()


# ---- groups, factors, tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis, factor", [("exp", 10.), ("cnn", 0.2), ("mlp", 1.), ("expmlp", 1.)])
def test_group_factors(basis, factor):
    f = OP.group_lr_factors(basis)
    gi = TU.GROUP_INDEX
    assert len(f) == G == 22
    expect = [1.] * G
    for n in ("nerf_beta_feat", "skin_aux", "ks"):
        expect[gi[n]] = 10.
    for n in ("nerf_root_rts", "root_code"):
        expect[gi[n]] = factor
    assert f == expect
    assert [gi["nerf_beta_feat"], gi["nerf_root_rts"], gi["root_code"], gi["skin_aux"], gi["ks"]] == [3, 10, 12, 18, 19]   # train_utils.py:262-284


def test_unknown_root_basis_is_refused():
    with pytest.raises(ValueError):
        OP.group_lr_factors("fourier")


HARNESS_NAMES = {       # what TrainHarness.named_params() produces (root_pose=True), by prefix -> group
    "nerf_coarse.xyz_encoding_1.0.weight": "nerf_coarse", "nerf_coarse.sigma.bias": "nerf_coarse", "nerf_coarse.beta": "nerf_beta",
    "nerf_skin.xyz_encoding_3.0.bias": "nerf_skin", "rest_pose_code.weight": "pose_code", "nerf_feat.rgb.0.weight": "nerf_feat",
    "nerf_feat.beta": "nerf_beta_feat", "nerf_vis.xyz_encoding_final.weight": "nerf_vis", "nerf_unc.rgb.0.bias": "nerf_unc",
    "bones": "bones", "skin_aux": "skin_aux", "nerf_root_rts.base_rt.se3": "nerf_root_rts",
    "nerf_root_rts.root_code.basis_mlp.weight": "nerf_root_rts", "nerf_root_rts.mlp_rt.xyz_encoding_1.0.weight": "nerf_root_rts",
}


def test_groups_of_the_harness_names_and_the_skipped_list():
    for n, g in HARNESS_NAMES.items():
        assert TU.grad_group(n) == TU.GROUP_INDEX[g], n
    named = [(n, torch.nn.Parameter(torch.zeros(3))) for n in list(HARNESS_NAMES) + ["mystery.weight", "module.module.bones"]]
    with pytest.raises(RuntimeError, match="CUDA"):           # grouping and validation are host work; the tables need the device
        OP.DeviceAdamW(named, 5e-4, 40, 0.2)
    groups = [TU.grad_group(n) for n, _ in named]
    assert [n for (n, _), g in zip(named, groups) if g is None] == ["mystery.weight", "module.module.bones"]
    with pytest.raises(ValueError, match="no parameter"):
        OP.DeviceAdamW([("mystery.weight", torch.nn.Parameter(torch.zeros(3)))], 5e-4, 40, 0.2)


def test_tables_over_the_segment_sizes():
    numels = [1, 5, 4096, 4097, 9000]
    chunk_seg, chunk_off, moff, n_state = OP.build_tables(numels)
    assert OP.CHUNK == 4096
    assert chunk_seg == [0, 1, 2, 3, 3, 4, 4, 4] and chunk_off == [0, 0, 0, 0, 4096, 0, 4096, 8192]
    assert moff == [0, 4, 12, 4108, 8208] and n_state == 8208 + 9000
    covered = [np.zeros(n, int) for n in numels]
    for s, off in zip(chunk_seg, chunk_off):
        covered[s][off:off + 4096] += 1
        assert off % 4096 == 0
    assert all((c == 1).all() for c in covered)
    for a, b, n in zip(moff, moff[1:] + [n_state], numels):
        assert a % 4 == 0 and b - a >= n
    assert OP.build_tables([]) == ([], [], [], 0)
    with pytest.raises(ValueError):
        OP.build_tables([3, 0])


# ---- bindings and refused tensors -------------------------------------------------------------------------------------------------
def test_new_entry_is_bound_and_declared():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    assert "moda_adamw_step" in _lib.EXPORTS and "moda_adamw_step" in declared and hasattr(lib, "moda_adamw_step")
    assert _lib.ABI_VERSION == 11 and lib.moda_abi_version() == 11          # purely additive: the number stays
    assert "purely additive" in hdr
    from moda_amd import build
    assert "optim_kernels.hip" in build.SOURCES
    import moda_amd
    assert moda_amd.DeviceAdamW is OP.DeviceAdamW and moda_amd.build_optimizer is OP.build_optimizer
    assert moda_amd.optimizer_step is OP.optimizer_step


def test_non_contiguous_and_non_fp32_tensors_are_refused_by_name():
    good = torch.nn.Parameter(torch.zeros(4, 4))
    strided = torch.nn.Parameter(torch.zeros(4, 8)[:, ::2])
    half = torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))
    assert not strided.is_contiguous()
    with pytest.raises(ValueError, match="nerf_coarse.a"):
        OP.DeviceAdamW([("bones", good), ("nerf_coarse.a", strided)], 5e-4, 40, 0.2)
    with pytest.raises(ValueError, match="nerf_skin.h"):
        OP.DeviceAdamW([("bones", good), ("nerf_skin.h", half)], 5e-4, 40, 0.2)
    OP.check_tensor("the gradient of", "bones", good.detach(), good.device)
    with pytest.raises(ValueError, match="the gradient of nerf_vis.g"):
        OP.check_tensor("the gradient of", "nerf_vis.g", torch.zeros(4, 8)[:, ::2], None)
    with pytest.raises(ValueError, match="the gradient of nerf_vis.d"):
        OP.check_tensor("the gradient of", "nerf_vis.d", torch.zeros(4, dtype=torch.float64), None)
    with pytest.raises(ValueError, match="nerf_vis.m"):
        OP.check_tensor("the gradient of", "nerf_vis.m", torch.zeros(4), torch.device("meta"))
