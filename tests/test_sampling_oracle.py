"""CPU: the float64 references of the samplers and the hierarchical resampling stage (tests/sampling_numpy.py) against
oracle/moda_oracle.py (`sample_pdf`, `sample_z`) run in float64, torch.linspace and torch.sort(stable=True); the case generators
tests/test_gpu_sampling.py runs on the device; and the conditions those cases must meet for its per-sample bars to be fair.

sample_pdf is a piecewise-linear map of u with one kind of discontinuity in its inputs and one in u:
  * a pdf entry crossing eps = 1e-5 switches its divisor between the entry and 1 (rendering.py:619).  Every float64 pdf entry
    of every case stays more than 1 % (relative) away from eps, so an fp32 evaluation cannot take the other side.
  * across a knot between two ordinary bins the map is continuous (either bin gives the same value there), but a bin that
    collapsed (pdf < eps, divisor 1) ends short of its right edge: the map JUMPS at both knots of a collapsed bin.  Only the
    `heavy` weights have such bins.  No sample -- no injected u and no point of the deterministic linspace grids -- lies within
    KNOT_TOL = 2^-20 of such a knot; KNOT_TOL is the distance under which the GPU test treats a sample as `at a knot`, 16 fp32
    ulps of the CDF's range.  The generator enforces it (weights of a heavy ray are redrawn, uniforms are redrawn); nothing is
    left out of the comparison.  Injected uniforms aimed at the MIDDLE of a collapsed bin (1.6e-6 from both its knots) keep the
    divisor-1 branch covered."""
import functools

import numpy as np
import pytest
import torch

import sampling_numpy as sn
from oracle import moda_oracle as orc

EPS = sn.EPS
U32 = 2.0 ** -24
KNOT_TOL = 2.0 ** -20
EPS_MARGIN = 0.01

# ---------------------------------------------------------------------------------------------------------------- sample_pdf cases
PDF_NW = (1, 2, 62, 63, 64, 65, 126, 127, 129, 254, 1023)      # pdf entries: 64-lane scan with 1, 2, 3, 4 and 16 entries per lane,
PDF_NIMP = (1, 2, 3, 64, 257)                                  # full / ragged / empty last runs; 257 > one workgroup of samples
PDF_KINDS = ("uniform", "sparse", "spike", "zero", "heavy")
RAYS_PER_KIND = 8
PDF_RAYS = RAYS_PER_KIND * len(PDF_KINDS)
TIED_NW = 65                                                   # the case whose bins have equal neighbours


def kind_rows(kind):
    k = PDF_KINDS.index(kind)
    return slice(k * RAYS_PER_KIND, (k + 1) * RAYS_PER_KIND)


def jump_knots(w_row):
    """CDF knots (float64) at which the map jumps: both ends of every collapsed bin of one ray."""
    pdf, cdf = sn.pdf_cdf64(w_row[None])
    c = np.nonzero(pdf[0] < EPS)[0]
    return np.unique(np.concatenate([cdf[0, c], cdf[0, c + 1]]))


def knot_distance(u, knots):
    """Distance of every u to the nearest of `knots` (inf when there are none)."""
    u = np.asarray(u, np.float64)
    if len(knots) == 0:
        return np.full(u.shape, np.inf)
    i = np.clip(np.searchsorted(knots, u), 1, len(knots) - 1) if len(knots) > 1 else np.zeros(u.shape, np.int64)
    lo = knots[np.maximum(i - 1, 0)]
    return np.minimum(np.abs(u - lo), np.abs(u - knots[i]))


def _det_grid():
    return np.unique(np.concatenate([sn.linspace01(n) for n in PDF_NIMP]))


def _sparse_row(rng, nw):
    w = rng.uniform(0.2, 1.0, nw)
    w[rng.uniform(size=nw) < 0.6] = 0.0
    if not w.any():
        w[rng.integers(nw)] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def pdf_inputs(nw, tied_bins=False):
    """-> bins (PDF_RAYS, nw + 1), w (PDF_RAYS, nw) float32; rows kind_rows(kind) hold RAYS_PER_KIND rays of each weight kind."""
    rng = np.random.default_rng(1000 + nw + (7 if tied_bins else 0))
    gaps = rng.uniform(0.2, 1.0, (PDF_RAYS, nw + 1))                # uneven but never tiny: distinct edges after rounding
    bins = (0.1 + 0.5 * np.cumsum(gaps, -1) / gaps.sum(-1, keepdims=True)).astype(np.float32)
    if tied_bins:                                  # zero-width bins: a run of four equal edges, and every ninth edge doubled
        bins[:, 10:14] = bins[:, 10:11]
        bins[:, 20::9] = bins[:, 19:-1:9]
        assert (np.diff(bins, axis=-1) >= 0).all()
    w = np.zeros((PDF_RAYS, nw), np.float64)
    grid = _det_grid()
    for r in range(RAYS_PER_KIND):
        x = rng.uniform(0.2, 1.0, nw)
        w[kind_rows("uniform")][r] = 0.9 * x / x.sum()                   # dense
        x = _sparse_row(rng, nw)
        w[kind_rows("sparse")][r] = 0.9 * x / x.sum()                    # 60 % zeros, sum 0.9 as composited weights
        w[kind_rows("spike")][r, rng.integers(nw)] = 0.7                 # one sample holds the surface
        for _ in range(400):                                             # heavy: sum 3, zero-weight bins collapse (0.33 eps)
            x = _sparse_row(rng, nw)
            x[0] = x[0] or 0.5                                           # the knots 0 and 1 stay ordinary
            x[-1] = x[-1] or 0.5
            x = (3.0 * x / x.sum()).astype(np.float32)
            if (knot_distance(grid, jump_knots(x)) > 2 * KNOT_TOL).all():
                break
        else:
            raise AssertionError(f"no heavy ray whose jumps avoid the linspace grids (nw={nw})")
        w[kind_rows("heavy")][r] = x
    return bins, w.astype(np.float32)


def _specials(w_row, rng):
    """The uniforms every ray must see: 0, 1, the largest float below 1, two fp32-rounded interior CDF knots between ordinary
    bins, and (heavy rays) the middle of a collapsed bin."""
    pdf, cdf = sn.pdf_cdf64(w_row[None])
    pdf, cdf = pdf[0], cdf[0]
    ok = pdf >= EPS
    out = [np.float32(0.0), np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(0.0))]
    inner = [i for i in range(1, len(pdf)) if ok[i - 1] and ok[i]]
    if inner:
        out += [np.float32(cdf[inner[len(inner) // 3]]), np.float32(cdf[inner[-1]])]
    coll = np.nonzero(~ok)[0]
    if len(coll):
        j = coll[rng.integers(len(coll))]
        out.append(np.float32(0.5 * (cdf[j] + cdf[j + 1])))
    return out


@functools.lru_cache(maxsize=None)
def pdf_uniforms(nw, n_imp, tied_bins=False):
    """Injected u (PDF_RAYS, n_imp) float32: random, with the specials of the ray in its first slots, rotated by the ray index so
    that even one sample per ray meets every special within the RAYS_PER_KIND rays of a kind."""
    _, w = pdf_inputs(nw, tied_bins)
    rng = np.random.default_rng(5000 + 17 * nw + n_imp)
    u = rng.uniform(size=(PDF_RAYS, n_imp)).astype(np.float32)
    u = np.minimum(u, np.nextafter(np.float32(1.0), np.float32(0.0)))
    for r in range(PDF_RAYS):
        knots = jump_knots(w[r])
        for _ in range(100):                                             # redraw what fell beside a jump
            bad = knot_distance(u[r], knots) <= 2 * KNOT_TOL
            if not bad.any():
                break
            u[r, bad] = rng.uniform(size=int(bad.sum())).astype(np.float32)
        sp = _specials(w[r], rng)
        for s in range(min(n_imp, len(sp))):
            u[r, s] = sp[(r + s) % len(sp)]
    return u


def pdf_ratio(got, bins, w, n_imp, u=None):
    """|got - ref| / scale per sample, against sample_pdf64 on the same inputs.  The output is bins_b + (u - cdf_b) / D * width:
    its fp32 error is the CDF's rounding amplified by width / D, plus the rounding of the result, so
    scale = 2^-24 (width_j / D_j + |ref|) with j, D from the float64 reference; where u is within KNOT_TOL of a float64 knot the
    larger amplification of the two bins that meet there counts (either bin is a correct choice at a knot)."""
    z, j, D = sn.sample_pdf64(bins, w, n_imp, u)
    pdf, cdf = sn.pdf_cdf64(w)
    nw = pdf.shape[1]
    b64 = np.asarray(bins, np.float64)
    one = np.ones_like(pdf[:, :1])
    amp_bin = np.concatenate([np.diff(b64, axis=-1), 0 * one], -1) / np.concatenate([np.where(pdf < EPS, 1.0, pdf), one], -1)
    uu = np.broadcast_to(sn.linspace01(n_imp), z.shape) if u is None else np.asarray(u, np.float64)
    take = lambda a, i: np.take_along_axis(a, i, 1)
    amp = take(amp_bin, j)
    assert np.allclose(take(np.diff(b64, axis=-1, append=b64[:, -1:]), j) / D, amp, rtol=1e-9, atol=0)
    left = (j > 0) & (uu - take(cdf, j) <= KNOT_TOL)
    amp = np.where(left, np.maximum(amp, take(amp_bin, np.maximum(j - 1, 0))), amp)
    jn = np.minimum(j + 1, nw)
    right = (j < nw) & (take(cdf, jn) - uu <= KNOT_TOL)
    amp = np.where(right, np.maximum(amp, take(amp_bin, jn)), amp)
    return np.abs(np.asarray(got, np.float64) - z) / (U32 * (amp + np.abs(z)))


def oracle32_ratio(bins, w, n_imp, u=None):
    """The same figure for oracle/moda_oracle.py::sample_pdf run in float32 (sequential cumsum): the yardstick of the GPU bar."""
    return pdf_ratio(orc.sample_pdf(np.asarray(bins, np.float32), np.asarray(w, np.float32), n_imp, u=u), bins, w, n_imp, u)


# ------------------------------------------------------------------------------------------------------------------- sampler cases
SAMPLER_S = (1, 2, 3, 4, 5, 8, 63, 64, 127, 128)
SAMPLER_N = 37
BLOCK = 256


@functools.lru_cache(maxsize=None)
def sampler_inputs(S):
    """rays_o, rays_d (N, 3), near, far (N,), u (N, S) float32.  Ray 5 has near == far; every ray's u holds an exact 0 and
    (S >= 2) an exact 1."""
    rng = np.random.default_rng(300 + S)
    N = SAMPLER_N
    ro = rng.normal(0, 0.3, (N, 3)).astype(np.float32)
    rd = rng.normal(0, 1.0, (N, 3)).astype(np.float32)
    near = rng.uniform(0.05, 0.3, N).astype(np.float32)
    far = (near + rng.uniform(0.1, 0.6, N)).astype(np.float32)
    far[5] = near[5]
    u = rng.uniform(size=(N, S)).astype(np.float32)
    for r in range(N):
        u[r, r % S] = r % 2 if S == 1 else 0.0
        if S >= 2:
            u[r, (r + 1) % S] = 1.0
    return ro, rd, near, far, u


# --------------------------------------------------------------------------------------------------------------------- merge cases
MERGE_TOTALS = (2, 3, 33, 64, 65, 129, 256, 257, 2047, 2048)
MERGE_ROWS = 8
SORTEDNESS = ((True, True), (True, False), (False, True), (False, False))


def merge_splits(total):
    """(La, Lb) pairs of a total length: one element on either side, halves, thirds."""
    s = {(1, total - 1), (total - 1, 1), (total // 2, total - total // 2), (max(1, total // 3), total - max(1, total // 3))}
    return sorted(p for p in s if p[0] >= 1 and p[1] >= 1)


def _ascending(x):
    return bool((x[:-1] <= x[1:]).all())


@functools.lru_cache(maxsize=None)
def merge_inputs(La, Lb, sort_a, sort_b):
    """a (MERGE_ROWS, La), b (MERGE_ROWS, Lb) float32.  Row 0: every key equal; row 1: only +0.0 and -0.0; row 2: {-1, -0.0,
    +0.0, 1}; rows 3-5: keys from a small set of integers (ties within a, within b and across them); rows 6-7: distinct random
    keys with a fifth of b copied from a.  A half asked to be sorted is sorted; one asked to be unsorted is reversed where
    chance left it ascending, so that (unless all its keys are equal or it has one element) it is not."""
    L = La + Lb
    rng = np.random.default_rng(7000 + 4 * (2049 * La + Lb) + 2 * sort_a + sort_b)
    cat = np.empty((MERGE_ROWS, L), np.float32)
    cat[0] = 0.25
    cat[1] = rng.choice(np.asarray([0.0, -0.0], np.float32), L)
    cat[2] = rng.choice(np.asarray([-1.0, -0.0, 0.0, 1.0], np.float32), L)
    cat[3:6] = rng.integers(0, max(2, L // 3), (3, L)).astype(np.float32) * np.float32(0.125)
    cat[3:6, La] = cat[3:6, 0]                                             # (a tie across the halves even when one has one key)
    cat[6:] = rng.permutation(8 * L)[: 2 * L].reshape(2, L).astype(np.float32) / np.float32(8 * L)
    n_tie = min(La, Lb // 5)
    if n_tie:
        cat[6:, La:La + n_tie] = cat[6:, :n_tie]
    a, b = cat[:, :La].copy(), cat[:, La:].copy()
    for half, want_sorted in ((a, sort_a), (b, sort_b)):
        for row in half:
            if want_sorted:
                row[:] = np.sort(row, kind="stable")
            elif _ascending(row):
                row[:] = row[::-1].copy()
    return a, b


# =========================================================================================================================== tests
def test_linspace_and_count_of_one_against_torch():
    """linspace01 == torch.linspace in float64 -- n == 1 gives [0.], which is what a single sample must use."""
    assert torch.linspace(0, 1, 1).tolist() == [0.0] and torch.linspace(0, 1, 1, dtype=torch.float64).tolist() == [0.0]
    for n in (1, 2, 3, 4, 5, 64, 257):
        assert np.abs(sn.linspace01(n) - torch.linspace(0, 1, n, dtype=torch.float64).numpy()).max() <= 2.0 ** -52, n
    near, far = np.asarray([0.25, 0.1], np.float32), np.asarray([0.75, 0.1], np.float32)
    for disp in (False, True):                            # one sample sits at near (not far), jittered or not
        for perturb, u in ((0.0, None), (1.0, np.asarray([[0.0], [1.0]], np.float32))):
            z = sn.sample_z(near, far, 1, disp, perturb, u)
            t = torch.linspace(0, 1, 1, dtype=torch.float64)
            n_, f_ = torch.from_numpy(near.astype(np.float64))[:, None], torch.from_numpy(far.astype(np.float64))[:, None]
            want = 1 / (1 / n_ * (1 - t) + 1 / f_ * t) if disp else n_ * (1 - t) + f_ * t
            assert np.allclose(z, want.numpy(), rtol=1e-15, atol=0) and np.allclose(z[:, 0], near.astype(np.float64), rtol=1e-15)
    bins, w = pdf_inputs(62)
    z, j, D = sn.sample_pdf64(bins, w, 1)                 # u = [0]: the first bin's left edge, not the last bin's right one
    assert np.array_equal(z[:, 0], bins[:, 0].astype(np.float64)) and (j == 0).all()


@pytest.mark.parametrize("S", SAMPLER_S)
def test_sample_z_and_points_against_the_oracle_in_float64(S):
    ro, rd, near, far, u = sampler_inputs(S)
    n64, f64 = near.astype(np.float64)[:, None], far.astype(np.float64)[:, None]
    for disp in (False, True):
        for perturb in (0.0, 0.5, 1.0):
            z = sn.sample_z(near, far, S, disp, perturb, u)
            want = orc.sample_z(n64, f64, S, disp, perturb, u.astype(np.float64))
            assert z.shape == (SAMPLER_N, S) and np.allclose(z, want, rtol=1e-14, atol=0), (S, disp, perturb)
    z = sn.sample_z(near, far, S)
    t = torch.linspace(0, 1, S, dtype=torch.float64).numpy()
    assert np.allclose(z, n64 * (1 - t) + f64 * t, rtol=1e-14, atol=0)
    p = sn.points(ro, rd, z)
    assert np.allclose(p, ro.astype(np.float64)[:, None] + rd.astype(np.float64)[:, None] * z[..., None], rtol=1e-15, atol=0)
    # the conditions of the GPU test: ragged last blocks in both kernels, the special uniforms, one degenerate ray
    assert (SAMPLER_N * S) % BLOCK != 0 and (S % 4 != 0 or (SAMPLER_N * (S // 4)) % BLOCK != 0)
    assert (u == 0).any(1).all() if S > 1 else ((u == 0).any() and (u == 1).any())
    assert S == 1 or (u == 1).any(1).all()
    assert near[5] == far[5] and (np.delete(far - near, 5) > 0.05).all() and near.min() > 0


def _pdf_cases():
    for nw in PDF_NW:
        for n_imp in PDF_NIMP:
            yield nw, n_imp, False
    for n_imp in (64, 257):
        yield TIED_NW, n_imp, True


@pytest.mark.parametrize("nw", PDF_NW)
def test_sample_pdf64_against_the_oracle_in_float64_and_the_input_conditions(nw):
    for tied in ((False, True) if nw == TIED_NW else (False,)):
        bins, w = pdf_inputs(nw, tied)
        pdf, cdf = sn.pdf_cdf64(w)
        # every pdf entry keeps 1 % from eps: the divisor switch cannot flip in fp32
        margin = float(np.abs(pdf / EPS - 1).min())
        assert margin > EPS_MARGIN, (nw, margin)
        assert (np.diff(bins, axis=-1) >= 0).all() and (tied == bool((np.diff(bins, axis=-1) == 0).any()))
        # the kinds are what they claim to be
        for kind, total in (("uniform", 0.9), ("sparse", 0.9), ("spike", 0.7), ("zero", 0.0), ("heavy", 3.0)):
            assert np.allclose(w[kind_rows(kind)].sum(-1), total, rtol=1e-5), (nw, kind)
        assert (w[kind_rows("uniform")] > 0).all() and (w[kind_rows("zero")] == 0).all()
        assert ((w[kind_rows("spike")] > 0).sum(-1) == 1).all()
        collapsed = pdf < EPS
        assert not collapsed[: kind_rows("heavy").start].any()
        if nw >= 62:
            assert 0.4 < (w[kind_rows("sparse")] == 0).mean() < 0.8 and collapsed[kind_rows("heavy")].any(1).all()
            assert np.allclose(pdf[kind_rows("heavy")][collapsed[kind_rows("heavy")]] / EPS, 1 / 3, rtol=0.02)
        for n_imp in (PDF_NIMP if not tied else (64, 257)):
            u = pdf_uniforms(nw, n_imp, tied)
            assert u.dtype == np.float32 and u.min() >= 0 and u.max() <= 1
            for uu in (None, u):
                z, j, D = sn.sample_pdf64(bins, w, n_imp, uu)
                u64 = None if uu is None else uu.astype(np.float64)
                want = orc.sample_pdf(bins.astype(np.float64), w.astype(np.float64), n_imp, u=u64)
                assert want.dtype == np.float64 and np.allclose(z, want, rtol=1e-12, atol=0), (nw, n_imp)
                assert (z >= bins[:, :1]).all() and (z <= bins[:, -1:]).all() and (D > 0).all()
                assert ((D == 1) | (D >= EPS)).all()
                # no sample beside a jump of the map (module docstring)
                ug = np.broadcast_to(sn.linspace01(n_imp), z.shape) if uu is None else u64
                for r in range(PDF_RAYS):
                    d = knot_distance(ug[r], jump_knots(w[r]))
                    assert (d > KNOT_TOL).all(), (nw, n_imp, r, float(d.min()))
                ratio = oracle32_ratio(bins, w, n_imp, uu)
                assert np.isfinite(ratio).all()
            # the specials are there: exact 0, exact 1, the float below 1, fp32-rounded interior knots, collapsed-bin middles
            below1 = np.nextafter(np.float32(1), np.float32(0))
            c32 = cdf.astype(np.float32)
            for kind in PDF_KINDS:
                rows = kind_rows(kind)
                uk = u[rows]
                assert (uk == 0).any() and (uk == 1).any() and (uk == below1).any(), (nw, n_imp, kind)
                at_knot = [(uk[r][:, None] == c32[rows][r][None, 1:-1]).any() for r in range(RAYS_PER_KIND)]
                assert nw < 62 or any(at_knot), (nw, n_imp, kind)
            if nw >= 62:                                   # the divisor-1 branch is taken by at least one injected sample
                _, _, D = sn.sample_pdf64(bins[kind_rows("heavy")], w[kind_rows("heavy")], n_imp, u[kind_rows("heavy")])
                inside = D == 1
                uh = u[kind_rows("heavy")]
                assert (inside & (uh < below1)).any(), (nw, n_imp)


def test_oracle32_ratio_is_a_usable_yardstick():
    """The float32 oracle's own per-sample figure on the dense rays of the recipe's shape: a handful of units (the scale is one
    rounding of the CDF, amplified), finite, and zero for the float64 reference itself."""
    bins, w = pdf_inputs(62)
    r = oracle32_ratio(bins, w, 64)
    assert 0 < r.max() < 200
    z, _, _ = sn.sample_pdf64(bins, w, 64)
    assert pdf_ratio(z, bins, w, 64).max() == 0


@pytest.mark.parametrize("total", MERGE_TOTALS)
def test_merge_with_origin_is_the_stable_sort_and_the_cases_have_their_ties(total):
    for La, Lb in merge_splits(total):
        assert La + Lb == total
        for sa, sb in SORTEDNESS:
            a, b = merge_inputs(La, Lb, sa, sb)
            assert a.shape == (MERGE_ROWS, La) and b.shape == (MERGE_ROWS, Lb) and np.isfinite(a).all() and np.isfinite(b).all()
            z, src = sn.merge_with_origin(a, b)
            cat = np.concatenate([a, b], -1)
            tz, ti = torch.sort(torch.from_numpy(cat), dim=-1, stable=True)
            assert np.array_equal(src, ti.numpy()) and np.array_equal(z.view(np.uint32), tz.numpy().view(np.uint32))
            # sortedness as asked: every row of a sorted half ascends; an unsorted half has rows that do not
            for half, want_sorted in ((a, sa), (b, sb)):
                asc = [_ascending(row) for row in half]
                if want_sorted or half.shape[1] == 1:
                    assert all(asc)
                else:
                    assert not any(asc[6:]) and (half.shape[1] < 8 or not any(asc[3:]))
            # ties: all-equal row, signed zeros, within a, within b, across
            assert (cat[0] == cat[0, 0]).all() and set(np.unique(cat[1].view(np.uint32))) <= {0, 0x80000000}
            if total >= 33:
                assert len(np.unique(cat[1].view(np.uint32))) == 2
                for row in (3, 4, 5):
                    assert len(np.unique(a[row])) < La or La == 1
                    assert len(np.unique(b[row])) < Lb or Lb == 1
                    assert np.intersect1d(a[row], b[row]).size > 0
            if min(La, Lb // 5) >= 1:
                assert np.intersect1d(a[6], b[6]).size >= min(La, Lb // 5)


def test_merge_splits_cover_one_element_halves():
    assert merge_splits(2) == [(1, 1)] and merge_splits(3) == [(1, 2), (2, 1)]
    for total in MERGE_TOTALS[2:]:
        s = merge_splits(total)
        assert (1, total - 1) in s and (total - 1, 1) in s and (total // 2, total - total // 2) in s
