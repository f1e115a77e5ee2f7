"""CPU (no GPU needed): the oracle of the whole-sequence route, tests/icpdev_numpy.py, pinned against tests/pointset_numpy.py
on single pairs; the per-element stopping rule on a batch against B single runs; the clouds of the ragged-search GPU test kept
inside check_nearest's 0.1 % cap; and the new entries in the header, the binding and the built library."""
import os
import re

import numpy as np
import pytest

import icpdev_numpy as icn
import pointset_numpy as psn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("moda_nn_fwd_ragged", "moda_icp_moments_ragged", "moda_sim3_apply_masked", "moda_icp_solve", "moda_icp_advance",
           "moda_seq_metrics")
U = 2.0 ** -24
# the clouds of tests/test_gpu_seq_eval.py::test_ragged_nearest (seed of x, seed of y), confirmed below
RAGGED_SEEDS = {1: (301, 302), 1025: (303, 304)}
RAGGED_LENS = (1, 1024, 1025)


def cloud(seed, *shape):
    return np.random.default_rng(seed).uniform(-1, 1, shape + (3,)).astype(np.float32)


def ragged_case(N):
    """x (3,N,3), y (3,1025,3) whose padding rows are copies of the cloud's first query: reading one would win with distance 0."""
    sx, sy = RAGGED_SEEDS[N]
    x, y = cloud(sx, 3, N), cloud(sy, 3, 1025)
    for b, n in enumerate(RAGGED_LENS):
        y[b, n:] = x[b, 0]
    return x, y


@pytest.mark.parametrize("N", [1, 1025])
def test_ragged_clouds_stay_inside_the_index_cap(N):
    x, y = ragged_case(N)
    for b, (dmin, imin, second) in enumerate(icn.nearest_ragged(x, y, RAGGED_LENS, with_second=True)):
        assert imin.max() < RAGGED_LENS[b]
        left_out = int((~(second > (1 + 10 * U) * dmin)).sum())
        assert left_out <= 1e-3 * N, (b, left_out)
        if RAGGED_LENS[b] < 1025:                                             # the padding would have won, had it been read
            assert psn.nearest(x[b], y[b])[0][0] == 0.0 and dmin[0] > 0.0


@pytest.mark.parametrize("scale,reflect", [(1.0, False), (1.1, False), (1.0, True)])
def test_solve_from_sums_is_align(scale, reflect):
    X, Y, subset, R, T = psn.icp_case(3, 5.0, scale=scale)
    Yn = Y[subset].astype(np.float64)
    Rs, Ts, ss, S = icn.solve(icn.moments(X, Yn), len(X), estimate_scale=scale != 1.0, allow_reflection=reflect)
    Ra, Ta, sa = psn.align(X.astype(np.float64), Yn, estimate_scale=scale != 1.0, allow_reflection=reflect)
    assert np.abs(Rs - Ra).max() <= 1e-12 and np.abs(Ts - Ta).max() <= 1e-12 and abs(ss - sa) <= 1e-12
    assert np.abs(Rs - R).max() <= 1e-5 and abs(ss - scale) <= 1e-5 and (np.diff(S) <= 0).all()


def test_batch_of_one_is_the_single_pair_icp():
    X, Y, subset, R, T = psn.icp_case(0, 5.0)
    want = psn.iterative_closest_point(X, Y)
    for per_element in (True, False):
        got = icn.icp_batch(X[None], [Y], per_element=per_element)
        assert got["iterations"][0] == len(want.t_history) and got["converged"][0] == want.converged
        assert np.array_equal(got["idx"][0], want.idx) and abs(got["rmse"][0] - want.rmse) <= 1e-12
        assert np.abs(got["R"][0] - want.RTs.R).max() <= 1e-12 and np.abs(got["T"][0] - want.RTs.T).max() <= 1e-12
    one = icn.icp_batch(X[None], [Y], max_iterations=1)
    assert one["iterations"] == [1] and one["converged"] == [False]


def stopping_batch():
    """Three clouds of 1500 points against targets of 1500: X == Y, a 5 degree motion, a 15 degree motion."""
    cases = [psn.icp_case(10, 0.0, n_y=1500, n_x=1500), psn.icp_case(11, 5.0, n_y=1500, n_x=1500),
             psn.icp_case(12, 15.0, n_y=1500, n_x=1500)]
    X = np.stack([cases[0][1]] + [c[0] for c in cases[1:]])
    Y = np.stack([c[1] for c in cases])
    return X, Y


def test_stopping_rules():
    X, Y = stopping_batch()
    singles = [icn.icp_batch(X[b:b + 1], Y[b:b + 1], per_element=True) for b in range(3)]
    per = icn.icp_batch(X, Y, per_element=True)
    for b in range(3):                                                        # per element: exactly the batch of one
        assert per["iterations"][b] == singles[b]["iterations"][0] and per["converged"][b]
        assert np.array_equal(per["Xt"][b], singles[b]["Xt"][0]) and per["rmse"][b] == singles[b]["rmse"][0]
    # X == Y: the rmse is rounding dust from the first iteration on; `relative` is 1 there by definition, so the rule can only
    # see it from the second (in float64 the dust need not shrink: the count is printed, not fixed)
    print("iterations", per["iterations"], "rmse", per["rmse"])
    assert per["rmse"][0] <= 1e-12 and per["iterations"][0] >= 2
    assert len(set(per["iterations"])) > 1
    both = icn.icp_batch(X, Y, per_element=False)                             # all elements: one common count, nobody early
    assert len(set(both["iterations"])) == 1 and all(both["converged"])
    assert both["iterations"][0] >= max(per["iterations"])


def test_metrics_row_and_summary():
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    gts = [(v[:300 + 30 * k] * 1.01 + 0.01 * k).astype(np.float32) for k in range(3)]
    frames, summ = icn.eval_sequence([v] * 3, gts)
    for f, g in zip(frames, gts):
        want = psn.eval_mesh(v, g)
        assert f["row"][0] == want["cd"] and [f["row"][k] for k in (1, 2, 3)] == [want["f001"], want["f002"], want["f005"]]
        p1, p2 = f["row"][4], f["row"][5]
        assert f["row"][1] == (0.0 if p1 + p2 == 0 else 2 * p1 * p2 / (p1 + p2))
    cds = [f["cd"] for f in frames]
    assert summ["cd_ave"] == np.mean(cds) and summ["cd_max"] == max(cds)
    assert summ["f002_min"] == min(f["f002"] for f in frames) and summ["f005_ave"] == np.mean([f["f005"] for f in frames])


def test_sequence_entries_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    from moda_amd import _lib, build
    assert "icpdev_kernels.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in include/moda_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not bound in moda_amd/_lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert lib.moda_abi_version() == _lib.ABI_VERSION                         # purely additive: the number stays
    # refusals that need no device: they come before any pointer is looked at
    assert lib.moda_nn_fwd_ragged(None, None, 1, 4, 0, None, None, None, None, None, None) == -2
    assert lib.moda_nn_fwd_ragged(None, None, 2, 4, 2 ** 30, None, None, None, None, None, None) == -2
    assert lib.moda_nn_fwd_ragged(None, None, 1, 0, 4, None, None, None, None, None, None) == 0
    assert lib.moda_nn_fwd_ragged(None, None, 1, 4, 4, None, None, None, None, None, None) == -1
    assert lib.moda_icp_moments_ragged(None, None, None, None, 1, 0, 4, None, None, None, None, None) == -2
    assert lib.moda_sim3_apply_masked(None, None, 0, 4, None, None, None) == -2
    assert lib.moda_icp_solve(None, 0, 4, 0, 0, 0, None, None, None) == -2
    assert lib.moda_icp_solve(None, 1, 4, 0, 0, 65, None, None, None) == -1
    assert lib.moda_icp_solve(None, 1, 4, 0, 0, 0, None, None, None) == -1
    assert lib.moda_icp_advance(None, 1, 0, 1e-6, 1, None, None, None, None, None, None, None) == -2
    assert lib.moda_icp_advance(None, 1, 4, 1e-6, 1, None, None, None, None, None, None, None) == -1
    assert lib.moda_seq_metrics(None, None, 1, 0, 4, None, None, None, None) == -2
    assert lib.moda_seq_metrics(None, None, 1, 4, 4, None, None, None, None) == -1
