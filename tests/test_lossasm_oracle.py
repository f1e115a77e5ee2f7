"""CPU (-m "not gpu"): the float64 restatements of tests/lossasm_numpy.py against what the reference's own functions gave
(tests/golden/g30_loss_assembly.npz, written by tests/golden/gen_golden_lossasm.py), the bindings of the new entries, and the
conditions on the inputs that tests/test_gpu_lossasm.py relies on (built here so that what is asserted here is what runs there)."""
import ctypes
import os
import re

import numpy as np
import pytest

import lossasm_cases as cases
import lossasm_numpy as ln
from moda_amd import _lib
from lossasm_cases import (assembly_case, frame_case, line_case_counts, line_case_random, root_case, threshold_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("moda_loss_filter_ws_bytes", "moda_loss_filter_line", "moda_loss_filter_frame", "moda_root_sm", "moda_loss_assembly")
POSITIVE_COUNTS = cases.POSITIVE_COUNTS


@pytest.fixture(scope="module")
def g30():
    return np.load(os.path.join(ROOT, "tests", "golden", "g30_loss_assembly.npz"))


# ---- the restatements against the reference's recorded results ---------------------------------------------------------------
def test_filter_line_restatement_equals_the_reference(g30):
    T, S, N = g30["line_shape"]
    state = np.zeros(T * S)
    for c in range(3):
        inv, _, _ = ln.loss_filter_line(state, g30[f"line{c}_errid"], g30[f"line{c}_frameid"], g30[f"line{c}_vals"], S)
        assert np.array_equal(inv, g30[f"line{c}_invalid"]), c
        assert np.array_equal(state, g30[f"line{c}_state"]), c
    assert g30["line1_invalid"].any() and not g30["line1_invalid"].all()


def test_filter_frame_restatement_equals_the_reference(g30):
    state = np.zeros(9)
    for c in range(3):
        x, m = g30[f"frame{c}_x"], g30[f"frame{c}_mask"]
        inv, flo_err, _ = ln.loss_filter_frame(state, x.reshape(len(x), -1), m.reshape(len(x), -1), g30[f"frame{c}_errid"])
        assert np.array_equal(flo_err, g30[f"frame{c}_flo_err"]), c
        assert np.array_equal(inv, g30[f"frame{c}_invalid"]), c
        assert np.array_equal(state, g30[f"frame{c}_state"]), c
    assert not g30["frame0_invalid"].any()                            # no history: the median is NaN and flags nothing
    assert g30["frame2_invalid"].any()


def test_root_sm_restatement_equals_the_reference(g30):
    rtk, off = g30["root_rtk"], tuple(int(v) for v in g30["root_offset"])
    ref = ln.root_sm(rtk, off, clamp32=False)
    assert abs(ref["loss"] - float(g30["root_loss_f64"])) < 1e-14 * abs(ref["loss"])
    assert np.abs(ref["grad"] - g30["root_grad_f64"]).max() < 1e-13 * np.abs(ref["grad"]).max()
    assert np.all(ref["grad"][:2] == 0) and np.all(ref["grad"][:, 3] == 0)          # a video of two frames has no triple
    # the reference's fp32 run lies within the derived fp32 bound of the float64 value (clamped at the fp32 bounds there)
    ref32 = ln.root_sm(rtk, off, clamp32=True)
    assert abs(float(g30["root_loss_f32"]) - ref32["loss"]) <= 4 * ln.root_sm_loss_bound(ref32)
    clamped = ref32["cos"] > ref32["hi"]
    assert clamped.sum() >= 1                                         # the identical poses
    assert np.allclose(ref32["angle"][clamped], np.arccos(ref32["hi"]), rtol=0, atol=0)
    # rot_angle on single steps
    mats = rtk[:, :3, :3].astype(np.float64)
    rel = mats[:-1] @ mats[1:].transpose(0, 2, 1)
    ang = np.arccos(np.clip((np.trace(rel, axis1=1, axis2=2) - 1) / 2, -1 + 1e-4, 1 - 1e-4))
    assert np.abs(ang - g30["rot_angle_f64"]).max() < 1e-12


def test_root_sm_gradient_restatement_against_finite_differences():
    rtk, off = root_case("videos")
    rtk, off = rtk[:12].astype(np.float64), (0, 2, 5, 12)
    ref = ln.root_sm(rtk, off, clamp32=False)
    rng = np.random.default_rng(0)
    for _ in range(12):
        f, i, j = rng.integers(2, 12), rng.integers(0, 3), rng.integers(0, 4)
        h = 1e-6
        p, m = rtk.copy(), rtk.copy()
        p[f, i, j] += h
        m[f, i, j] -= h
        fd = (ln.root_sm(p, off, False)["loss"] - ln.root_sm(m, off, False)["loss"]) / (2 * h)
        assert abs(fd - ref["grad"][f, i, j]) < 1e-8 + 1e-6 * abs(fd), (f, i, j)


def test_assembly_restatement_gradient_against_finite_differences():
    rendered, opts = assembly_case()
    inv = np.zeros(37, bool)
    inv[[3, 20]] = True
    kw = dict(invalid=inv, progress=0.17, loss_select=1, root_sm_loss=0.25)
    total, aux, grads = ln.forward_default(rendered, opts, **kw)
    rng = np.random.default_rng(1)
    for key in ("img_loss_samp", "sil_loss_samp", "flo_loss_samp", "proj_err", "frame_cyc_dis", "vis_loss", "corr_err"):
        for _ in range(4):
            idx = tuple(rng.integers(0, s) for s in np.shape(rendered[key]))
            p = {k: np.array(v, np.float64 if np.asarray(v).dtype.kind == "f" else None) for k, v in rendered.items()}
            m = {k: v.copy() for k, v in p.items()}
            p[key][idx] += 1e-6
            m[key][idx] -= 1e-6
            fd = (ln.forward_default(p, opts, **kw)[0] - ln.forward_default(m, opts, **kw)[0]) / 2e-6
            assert abs(fd - grads[key][idx]) < 1e-9 + 1e-6 * abs(fd), (key, idx)
    assert grads["img_loss_samp"][3].max() == 0 and grads["proj_err"][20].max() == 0       # rejected rows


# ---- conditions on the inputs of the GPU tests -------------------------------------------------------------------------------
def test_threshold_pair_sits_on_and_one_step_above_ten_medians():
    for above in (False, True):
        T, S, errid, frameid, vals = threshold_case(above)
        inv, mean, med = ln.loss_filter_line(np.zeros(T * S), errid, frameid, vals, S)
        assert mean[3] == 10 * med if not above else mean[3] > 10 * med
        assert inv.tolist() == [False, False, False, above]


@pytest.mark.parametrize("K", POSITIVE_COUNTS)
def test_count_cases_have_the_stated_number_of_positive_frames(K):
    T, S, errid, frameid, vals = line_case_counts(K)
    inv, mean, med = ln.loss_filter_line(np.zeros(T * S), errid, frameid, vals, S)
    assert (mean > 0).sum() == K
    assert np.isnan(med) == (K == 0)
    assert inv.any() == (K >= 3)


def test_random_inputs_keep_clear_of_the_threshold():
    T, S, errid, frameid, vals = line_case_random()
    inv, mean, med = ln.loss_filter_line(np.zeros(T * S), errid, frameid, vals, S)
    assert np.abs(mean - 10 * med).min() > 1e-12 * 10 * med
    assert inv.any() and not inv.all()


@pytest.mark.parametrize("bs", [1, 5])
def test_frame_cases_meet_their_conditions(bs):
    for above in (False, True):
        T, hist, x, mask, errid = cases.frame_threshold_case(bs, above)
        inv, flo_err, med = ln.loss_filter_frame(hist.astype(np.float64), x, mask, errid)
        assert (float(flo_err[0]) == 10 * med) if not above else (float(flo_err[0]) > 10 * med)
        assert inv.tolist() == [above] + [False] * (bs - 1)
    T, hist, x, mask, errid = cases.frame_case_random(bs)
    inv, flo_err, med = ln.loss_filter_frame(hist.astype(np.float64), x, mask, errid)
    assert np.abs(flo_err.astype(np.float64) - 10 * med).min() > 1e-5 * 10 * med      # far wider than fp32 rounding of flo_err
    assert inv[0] and (bs == 1 or not inv.all())
    for K in POSITIVE_COUNTS:
        T, hist, *_ = frame_case(bs, K)
        assert (hist > 0).sum() == K


def test_root_cases_meet_their_conditions():
    rtk, off = root_case("videos")
    ref = ln.root_sm(rtk, off)
    assert len(ref["first"]) == 0 + 1 + 3 + 62 + 63 + 68
    edge = (np.abs(ref["cos"] - ref["lo"]) <= ref["cos_bound"]) | (np.abs(ref["cos"] - ref["hi"]) <= ref["cos_bound"])
    assert edge.mean() <= 0.02
    same = ln.root_sm(*root_case("same"))
    assert np.all(same["cos"] == 1) and np.all(same["trn"] == 0) and np.all(same["grad"] == 0)
    assert np.all(same["angle"] == np.arccos(float(np.float32(1 - 1e-4))))
    flip = ln.root_sm(*root_case("flip"))
    assert flip["cos"][0] == -1 and flip["angle"][0] == np.arccos(float(np.float32(-1 + 1e-4)))
    assert np.isnan(ln.root_sm(np.zeros((4, 4, 4)), (0, 2, 4))["loss"])


# ---- bindings ----------------------------------------------------------------------------------------------------------------
def test_new_entries_are_bound_and_declared():
    hdr = open(os.path.join(ROOT, "include", "moda_hip.h")).read()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS and name in declared, name
    assert _lib.ABI_VERSION == 11 and _lib.load().moda_abi_version() == 11
    assert ctypes.sizeof(_lib.AsmTerm) == 64
    from moda_amd import build
    assert "lossasm_kernels.hip" in build.SOURCES


def test_entries_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    EINVAL = -1
    assert lib.moda_loss_filter_ws_bytes(7, 8) == 8 * 7 + 4 * 56 + 8
    assert lib.moda_loss_filter_ws_bytes(0, 8) == 0
    assert lib.moda_loss_filter_line(None, None, 0, None, 0, 24, None, 7, 8, 10.0, None, None, None, None) == EINVAL
    assert lib.moda_loss_filter_frame(None, None, 0, 1, 8, None, 7, None, 0, 10.0, None, None, None, None) == EINVAL
    assert lib.moda_root_sm(None, 4, 10, None, 1, None, None, None, None) == EINVAL
    assert lib.moda_loss_assembly(None, 1, 1.0, None, None, None) == EINVAL
    arr = (_lib.AsmTerm * 17)()
    out = (ctypes.c_float * 64)()
    assert lib.moda_loss_assembly(arr, 17, 1.0, out, None, None) == EINVAL                 # more than 16 terms
    assert lib.moda_loss_assembly(arr, 1, 1.0, out, None, None) == EINVAL                  # a term without values


def test_forward_loss_refuses_the_flags_it_does_not_implement():
    from moda_amd import loss_utils as LU
    for opts, flag in ((dict(), "bone_loc_reg"), (dict(bone_loc_reg=0, ft_cse=True), "ft_cse"),
                       (dict(bone_loc_reg=0, freeze_coarse=True), "freeze_coarse")):
        with pytest.raises(NotImplementedError, match=flag):
            LU.forward_loss({}, opts)
    assert LU.LOSS_OPTS["loss_flt"] and LU.LOSS_OPTS["rm_novp"] and LU.LOSS_OPTS["root_sm"]   # moda.py:164-168
    assert LU.proj_warmup_weight(0.19, 0.0, 0.2) == float(np.clip((0.19 / 0.2 - 0.8) * 5, 0, 1))
    assert "REDUCED" in LU.total_loss.__doc__ and "default configuration" not in LU.total_loss.__doc__
