"""CPU (no GPU needed): the float64 oracle tests/pointset_numpy.py against the reference's recorded fscore (G28), the oracle's
ICP on a known rigid motion, and the presence of the point-set entries in the header, the binding and the built library."""
import os
import re

import numpy as np
import pytest

import pointset_numpy as psn
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("moda_nn_fwd", "moda_chamfer_bwd", "moda_icp_moments")


def test_oracle_fscore_matches_reference_fixture():
    g = golden("g28_fscore")
    zero = 0
    for name in g["cases"].tolist():
        d1, d2 = g[f"{name}_dist1"], g[f"{name}_dist2"]
        for k, thr in enumerate(g[f"{name}_thresholds"].tolist()):
            f, p1, p2 = psn.fscore(d1, d2, thr)
            # counts over sizes: float32 in the fixture, float64 here
            assert np.array_equal(p1.astype(np.float32), g[f"{name}_precision_1"][k])
            assert np.array_equal(p2.astype(np.float32), g[f"{name}_precision_2"][k])
            assert np.abs(f - g[f"{name}_fscore"][k]).max() <= 2 ** -22
            both = (g[f"{name}_precision_1"][k] == 0) & (g[f"{name}_precision_2"][k] == 0)
            assert (f[both] == 0).all() and (g[f"{name}_fscore"][k][both] == 0).all()
            zero += int(both.sum())
    assert zero >= 1                                                          # the 0/0 rule is exercised
    assert np.abs(psn.fscore(g["a_dist1"], g["a_dist2"])[0] - g["default_threshold_fscore"]).max() <= 2 ** -22


def test_oracle_nearest_tie_rule_and_second():
    y = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0], [5, 5, 5]], np.float32)
    x = np.array([[0.1, 0, 0], [0.9, 0, 0], [4, 4, 4]], np.float32)
    d, i, s = psn.nearest(x, y, with_second=True)
    assert i.tolist() == [0, 1, 4] and np.allclose(d, [0.1 ** 2, 0.1 ** 2, 3.0], rtol=1e-6)
    assert np.allclose(s[:2], d[:2])                                          # the duplicate is the runner-up
    d1, i1 = psn.nearest(x, y, chunk=1)
    assert np.array_equal(i1, i) and np.array_equal(d1, d)


@pytest.mark.parametrize("seed,degrees", [(0, 5.0), (1, 10.0), (2, 15.0)])
def test_oracle_icp_recovers_known_motion(seed, degrees):
    X, Y, subset, R, T = psn.icp_case(seed, degrees)
    sol = psn.iterative_closest_point(X, Y)
    assert sol.converged and len(sol.t_history) < 100
    assert np.array_equal(sol.idx, subset)                                    # every correspondence is the true one
    bbox = float((Y.max(0) - Y.min(0)).max())
    print(seed, degrees, "iterations", len(sol.t_history), "rmse", sol.rmse)
    assert sol.rmse <= 1e-5 * bbox
    assert np.abs(sol.RTs.R - R).max() <= 1e-5 and np.abs(sol.RTs.T - T).max() <= 1e-5 and sol.RTs.s == 1.0


def test_oracle_icp_scale_and_iteration_limit():
    X, Y, subset, R, T = psn.icp_case(3, 5.0, scale=1.1)
    sol = psn.iterative_closest_point(X, Y, estimate_scale=True)
    assert sol.converged and np.array_equal(sol.idx, subset) and abs(sol.RTs.s - 1.1) <= 1e-5
    one = psn.iterative_closest_point(X, Y, max_iterations=1)
    assert not one.converged and len(one.t_history) == 1


def test_oracle_chamfer_gradient_is_the_derivative():
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((40, 3)), rng.standard_normal((55, 3))
    g1, g2 = rng.standard_normal(40), rng.standard_normal(55)
    d1, d2, i1, i2 = psn.chamfer(x, y)
    gx, gy, *_ = psn.chamfer_grad(x, y, i1, i2, g1, g2)

    def loss(x_, y_):
        a, b, _, _ = psn.chamfer(x_, y_)
        return (g1 * a).sum() + (g2 * b).sum()
    h = 1e-6
    for arr, grad, which in ((x, gx, 0), (y, gy, 1)):
        for (r, c) in ((0, 0), (7, 2), (20, 1)):
            p = arr.copy()
            p[r, c] += h
            m = arr.copy()
            m[r, c] -= h
            num = (loss(p, y) - loss(m, y)) / (2 * h) if which == 0 else (loss(x, p) - loss(x, m)) / (2 * h)
            assert abs(num - grad[r, c]) <= 1e-6 * max(1.0, abs(num))


def test_point_set_entries_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    from moda_amd import _lib, build
    assert "pointset_kernels.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in include/moda_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not bound in moda_amd/_lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert lib.moda_abi_version() == _lib.ABI_VERSION == 11
    # shape refusals need no device: they come before any pointer is looked at
    assert lib.moda_nn_fwd(None, None, 1, 4, 0, None, None, None, None) == -2
    assert lib.moda_nn_fwd(None, None, 0, 4, 4, None, None, None, None) == -2
    assert lib.moda_nn_fwd(None, None, 2, 2 ** 30, 4, None, None, None, None) == -2
    assert lib.moda_nn_fwd(None, None, 2, 4, 2 ** 30, None, None, None, None) == -2
    assert lib.moda_nn_fwd(None, None, 1, 0, 4, None, None, None, None) == 0
    assert lib.moda_chamfer_bwd(None, None, None, None, 1, 4, 0, None, None, None) == -2
    assert lib.moda_icp_moments(None, None, None, None, 2, 2 ** 30, 4, None, None, None) == -2
