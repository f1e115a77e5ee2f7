"""GPU (-m gpu): the ray samplers and the hierarchical resampling stage (csrc/render_kernels.hip: sample_rays / sample_rays4 / points,
sample_pdf, merge_index, merge_rows, merge_sort) against the float64 references of tests/sampling_numpy.py, on the cases
tests/test_sampling_oracle.py builds and vets on the CPU.  u = 2^-24 (fp32 unit round-off) below.

sample_pdf   The CDF is built by one 64-lane wave, each lane summing `per = ceil(nw / 64)` consecutive entries, the runs joined by
             a shuffle scan.  nw in {1, 2, 62, 63, 64, 65, 126, 127, 129, 254, 1023} gives per = 1, 2, 3, 4, 16 with full, ragged
             and empty last runs (nb = 1024 is the entry point's limit); n_imp in {1, 2, 3, 64, 257} (257: the sample loop
             strides); deterministic u and injected u holding exact 0, exact 1, the float below 1, fp32-rounded interior CDF
             knots and (heavy rays) the middle of a collapsed bin; five weight kinds per shape (8 rays each, one launch); one
             shape whose bins have equal neighbours.
             Compared PER SAMPLE (a relative L2 hides one sample in the wrong bin): |got - ref| / scale with
             scale = u (width_j / D_j + |ref|), j and D the float64 reference's bin and divisor, the larger of the two adjacent
             bins within 2^-20 of a float64 knot (test_sampling_oracle.pdf_ratio).  Bar per (shape, kind, mode): the larger of 4
             (the four roundings of the interpolation) and 4 x the worst figure oracle/moda_oracle.py::sample_pdf reaches in
             float32 on the same inputs, computed here at run time from the oracle.  The margin of 4 covers the kernel's
             different association of the sum (lane runs + scan against numpy's sequential cumsum).
             Measured on an MI355X, 570 (shape, kind, mode) cases, worst |got - ref| / scale of the kernel with the float32
             oracle's figure on the same case:
               kind      kernel   oracle32   at (nw, n_imp, mode)          by nw (kernel / oracle32, worst kind):
               uniform     2.59       6.69   1023, 257, det                   1  0.87 / 0.93     126   1.93 / 17.4
               sparse      3.84       87.9   1023, 257, u                     2  1.00 / 1.05     127   2.08 / 33.7
               spike      12.79      170.7   1023, 257, det                  63  1.79 / 14.5     129   3.06 / 27.8
               zero        1.93       17.4   126, 64, det                    65  2.25 / 24.6     254   2.59 / 43.7
               heavy       2.90       27.4   1023, 64, det                 62, 64  1.98 (sparse)  1023  12.79 / 170.7
             Only the spike rays at nw = 1023 pass 4 (7.7 to 12.8: sixteen entries per lane, and the spike's bin divides by a
             pdf of 1e-5 / 0.71), where the sequential float32 oracle is at 159 to 207; everywhere else the kernel is under 4.  In
             26 small cases the kernel's figure is above the oracle's (both under 2).  With injected u on the heavy rays the
             oracle's own figure reaches 1.8e4 in some cases: the uniform aimed at the middle of a collapsed bin (3.3e-6 wide in
             u) lands in the neighbouring bin under its sequential CDF, so there the bar is set by the oracle's bin choice and
             says little; the kernel takes the float64 bin on every such sample (worst heavy figure 2.90).
             Samplers, worst |dz| / bar: 0.25 (S = 128, linear, no jitter); end-to-end case below: 1.5e-6 (depth_rnd).
samplers     S in {1, 2, 3, 4, 5, 8, 63, 64, 127, 128}, N = 37 rays (N S and N S / 4 leave ragged last blocks), linear and
             disparity depths, perturb 0 / 0.5 / 1 with u holding exact 0 and 1, one ray with near == far, output buffers
             16-byte aligned (four samples per thread where S % 4 == 0) and 4 bytes off (one sample per thread): the two bit for
             bit equal.  Bars, with m = max(|near|, |far|) of the ray:
               t          step = fl(1 / (S - 1)) and one product (lower half) or a product and a subtraction from 1 (upper half):
                          |dt| <= 2 u; 1 - t rounds once more: 3 u.
               linear     near (1 - t) + far t: 3 u |near| + 2 u |far| from the operands, one rounding per product and one for
                          the sum, all <= u m: |dz| <= 8 u m.
               disparity  d = (1 / near)(1 - t) + (1 / far) t the same with one more rounding for each reciprocal: |dd| <= 10 u
                          max(1 / near, 1 / far); z = 1 / d rounds once and d >= min(1 / near, 1 / far), so |dz| <=
                          (10 k + 1) u |z| with k = max(near, far) / min(near, far); |z| <= m.
               jitter     lower + (upper - lower) (perturb u): lower and upper are half-sums of two depths (each E = the bar
                          above, one rounding more: E + u m), their difference carries both, the product of two factors <= 1
                          rounds twice and the sum once: |dz| <= 3 (E + u m) + 4 u m.
               points     o + d z from the kernel's own fp32 z: one rounding of the product, one of the sum (none where the
                          compiler contracts them): |dp| <= u (2 |d z| + |o|).
             Bit-exact with perturb == 0: linear z[:, 0] == near and (S >= 2) z[:, -1] == far (t is exactly 0 and 1 there and
             x * 0 + y == y for positive operands); disparity ends == fl(1 / fl(1 / near)), fl(1 / fl(1 / far)); S == 1: the single
             depth is the near end (torch.linspace(0, 1, 1) == [0.]).
merges       merge_index: src == the stable argsort of cat(a, b) exactly (equal keys: a before b, then the lower index), z ==
             cat[src] bit for bit -- all four sortedness combinations (binary-search and counting rank paths of either half),
             totals {2, 3, 33, 64, 65, 129, 256, 257, 2047, 2048} split 1 + (L - 1), (L - 1) + 1, halves and thirds, rows of
             equal keys, of +0.0 / -0.0, ties within and across the halves.  merge_rows gathers C in {1, 3, 4, 5, 64} channels by
             that origin, exactly.  merge_sort at the same lengths and with Lb == 0: non-decreasing, the input's multiset of bit
             patterns.
refusals     nb = 1, nb = 1025, La + Lb = 2049, C = 65: an error, and the output buffers keep their bytes.
end to end   render_rays(use_fine=True, N_samples=256, perturb=0) -- 128 + 128 samples, nw = 126, two entries per lane -- on 6
             rays without bones, fp32, against oracle.render_rays at the bar of test_gpu_parity.test_shape_sweep_against_oracle
             (1e-4 of the tensor's largest magnitude) on its keys (a scene without bones has no canonical points or cycle
             distance: the camera-frame points of the merged depths stand in for them)."""
import numpy as np
import pytest
import torch

import sampling_numpy as sn
import test_sampling_oracle as C
from helpers import oracle_scene, rel_err

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import _lib as L, rendering as R, synth
    from oracle import moda_oracle as orc
    from gpu_helpers import T, DEV, make_models, make_opts, rays_to_gpu

U = 2.0 ** -24


def np_(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(autouse=True)
def _no_grad_fp32():
    moda_amd.set_precision("fp32")
    with torch.no_grad():
        yield
    moda_amd.set_precision("fp32")


# ------------------------------------------------------------------------------------------------------------------------ sample_pdf
def _check_pdf(nw, n_imp, tied=False):
    bins, w = C.pdf_inputs(nw, tied)
    u = C.pdf_uniforms(nw, n_imp, tied)
    for mode, uu in (("det", None), ("u", u)):
        got = np_(R.sample_pdf(T(bins), T(w), n_imp, det=uu is None, u=None if uu is None else T(uu)))
        assert got.shape == (C.PDF_RAYS, n_imp) and got.dtype == np.float32
        ratio = C.pdf_ratio(got, bins, w, n_imp, uu)
        ref = C.oracle32_ratio(bins, w, n_imp, uu)
        for kind in C.PDF_KINDS:
            rows = C.kind_rows(kind)
            k, o = float(ratio[rows].max()), float(ref[rows].max())
            print(f"sample_pdf nw={nw} n_imp={n_imp} {mode} {kind}{' tied-bins' if tied else ''}: kernel {k:.2f} oracle32 {o:.2f}")
            assert k <= max(4.0, 4.0 * o), (nw, n_imp, mode, kind, k, o, np.unravel_index(np.argmax(ratio[rows]), ratio[rows].shape))


@pytest.mark.parametrize("nw", C.PDF_NW)
def test_sample_pdf_per_sample_against_float64(nw):
    for n_imp in C.PDF_NIMP:
        _check_pdf(nw, n_imp)


def test_sample_pdf_with_zero_width_bins():
    for n_imp in (64, 257):
        _check_pdf(C.TIED_NW, n_imp, tied=True)


def test_one_importance_sample_is_the_first_bin_edge():
    """det=True with n_imp = 1 is u = linspace(0, 1, 1) = [0.]: the left edge of the first bin, bit for bit."""
    bins, w = C.pdf_inputs(62)
    got = np_(R.sample_pdf(T(bins), T(w), 1, det=True))
    assert np.array_equal(bits(got[:, 0]), bits(bins[:, 0]))


# -------------------------------------------------------------------------------------------------------------------------- samplers
def _run_samplers(ro, rd, near, far, u, perturb, use_disp, S, off):
    """moda_sample_rays_fwd + moda_points_fwd into buffers that start `off` floats past a 16-byte boundary."""
    N = ro.shape[0]
    zb = torch.full((N * S + 4,), 7.0, device=DEV)
    xb = torch.full((N * S * 3 + 4,), 7.0, device=DEV)
    x2b = torch.full((N * S * 3 + 4,), 7.0, device=DEV)
    z, x, x2 = zb[off:off + N * S], xb[off:off + N * S * 3], x2b[off:off + N * S * 3]
    assert z.data_ptr() % 16 == 4 * off and x.data_ptr() % 16 == 4 * off
    L.call("moda_sample_rays_fwd", L.ptr(ro), L.ptr(rd), L.ptr(near), L.ptr(far), L.ptr(u), float(perturb), int(use_disp), N, S,
           z.data_ptr(), x.data_ptr(), L.stream())
    zc = z.clone() if off == 0 else z                        # (the clone is 16-byte aligned; the view is not)
    L.call("moda_points_fwd", L.ptr(ro), L.ptr(rd), zc.data_ptr(), N, S, x2.data_ptr(), L.stream())
    out = np_(z).reshape(N, S), np_(x).reshape(N, S, 3), np_(x2).reshape(N, S, 3)
    for buf, used in ((zb, N * S), (xb, N * S * 3), (x2b, N * S * 3)):      # nothing written outside the view
        assert bool((buf[:off] == 7.0).all()) and bool((buf[off + used:] == 7.0).all())
    return out


@pytest.mark.parametrize("S", C.SAMPLER_S)
def test_samplers_and_points_against_float64(S):
    ro, rd, near, far, u = C.sampler_inputs(S)
    N = C.SAMPLER_N
    dev = [T(x) for x in (ro, rd, near, far, u)]
    m = np.maximum(np.abs(near), np.abs(far)).astype(np.float64)[:, None]
    kappa = (np.maximum(near, far) / np.minimum(near, far)).astype(np.float64)[:, None]
    one = np.float32(1.0)
    for use_disp in (0, 1):
        E = (10 * kappa + 1) * U * m if use_disp else 8 * U * m          # unjittered depths (module docstring)
        for perturb in (0.0, 0.5, 1.0):
            bar = E if perturb == 0 else 3 * (E + U * m) + 4 * U * m
            ref = sn.sample_z(near, far, S, bool(use_disp), perturb, u)
            outs = [_run_samplers(*dev[:4], dev[4] if perturb > 0 else None, perturb, use_disp, S, off) for off in (0, 1)]
            for a, b in zip(*outs):                                      # four samples per thread == one sample per thread
                assert np.array_equal(bits(a), bits(b)), (S, use_disp, perturb)
            z, x, x2 = outs[0]
            err = np.abs(z.astype(np.float64) - ref) / bar
            print(f"samplers S={S} disp={use_disp} perturb={perturb}: worst |dz| / bar {err.max():.3f}")
            assert err.max() <= 1, (S, use_disp, perturb, float(err.max()))
            p = sn.points(ro, rd, z)
            dz = np.abs(rd.astype(np.float64)[:, None, :] * z.astype(np.float64)[:, :, None])
            pbar = U * (2 * dz + np.abs(ro.astype(np.float64))[:, None, :])
            for got in (x, x2):
                assert (np.abs(got.astype(np.float64) - p) <= pbar).all(), (S, use_disp, perturb)
            if perturb == 0:
                lo, hi = (one / (one / near), one / (one / far)) if use_disp else (near, far)
                assert np.array_equal(bits(z[:, 0]), bits(lo)), (S, use_disp)           # S == 1: the near end
                if S >= 2:
                    assert np.array_equal(bits(z[:, -1]), bits(hi)), (S, use_disp)
            elif S == 1:                                                 # one stratum of zero width: jitter moves nothing
                assert np.array_equal(bits(z[:, 0]), bits(one / (one / near) if use_disp else near))


# ---------------------------------------------------------------------------------------------------------------------------- merges
@pytest.mark.parametrize("total", C.MERGE_TOTALS)
def test_merge_index_is_the_stable_argsort(total):
    for La, Lb in C.merge_splits(total):
        for sa, sb in C.SORTEDNESS:
            a, b = C.merge_inputs(La, Lb, sa, sb)
            want_z, want_src = sn.merge_with_origin(a, b)
            z, src = R._merge_index(T(a), T(b))
            assert src.dtype == torch.int32
            assert np.array_equal(np_(src).astype(np.int64), want_src), (La, Lb, sa, sb)
            assert np.array_equal(bits(np_(z)), bits(want_z)), (La, Lb, sa, sb)


@pytest.mark.parametrize("c", [1, 3, 4, 5, 64])
def test_merge_rows_gathers_by_origin(c):
    rng = np.random.default_rng(90 + c)
    for La, Lb in ((40, 25), (1, 32), (128, 129)):
        a, b = C.merge_inputs(La, Lb, True, False)
        _, src = R._merge_index(T(a), T(b))
        ra = rng.normal(size=(C.MERGE_ROWS, La, c)).astype(np.float32)
        rb = rng.normal(size=(C.MERGE_ROWS, Lb, c)).astype(np.float32)
        got = np_(R._merge_rows(src, T(ra), T(rb)))
        _, want_src = sn.merge_with_origin(a, b)
        want = np.take_along_axis(np.concatenate([ra, rb], 1), want_src[..., None].repeat(c, 2), 1)
        assert np.array_equal(bits(got), bits(want)), (c, La, Lb)


@pytest.mark.parametrize("total", C.MERGE_TOTALS)
def test_merge_sort_keeps_the_bit_patterns_in_order(total):
    for La, Lb in C.merge_splits(total) + [(total, 0)]:
        for sa, sb in C.SORTEDNESS:
            if Lb == 0:
                a, _ = C.merge_inputs(total, 1, sa, True)
                b = np.zeros((C.MERGE_ROWS, 0), np.float32)
            else:
                a, b = C.merge_inputs(La, Lb, sa, sb)
            got = np_(R._merge_sorted(T(a), T(b)))
            assert got.shape == (C.MERGE_ROWS, total)
            assert (got[:, :-1] <= got[:, 1:]).all(), (La, Lb, sa, sb)
            cat = np.concatenate([a, b], -1)
            assert np.array_equal(np.sort(bits(got), -1), np.sort(bits(cat), -1)), (La, Lb, sa, sb)


# -------------------------------------------------------------------------------------------------------------------------- refusals
def test_out_of_range_shapes_are_refused_and_nothing_is_written():
    n = 4
    f = lambda *shape: torch.full(shape, 3.0, device=DEV)
    for nb in (1, 1025):
        out = f(n, 8)
        with pytest.raises(RuntimeError):
            L.call("moda_sample_pdf_fwd", L.ptr(f(n, nb)), L.ptr(f(n, max(nb - 1, 1))), None, n, nb, 8, L.ptr(out), L.stream())
        with pytest.raises(RuntimeError):
            R.sample_pdf(f(n, nb), f(n, nb - 1), 8, det=True)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all())
    a, b = f(n, 1024), f(n, 1025)
    z, src = f(n, 2049), torch.full((n, 2049), 5, device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        L.call("moda_merge_index_fwd", L.ptr(a), 1024, L.ptr(b), 1025, n, L.ptr(z), L.ptr(src), L.stream())
    with pytest.raises(RuntimeError):
        L.call("moda_merge_sort_fwd", L.ptr(a), 1024, L.ptr(b), 1025, n, L.ptr(z), L.stream())
    with pytest.raises(RuntimeError):
        R._merge_index(a, b)
    with pytest.raises(RuntimeError):
        R._merge_sorted(a, b)
    torch.cuda.synchronize()
    assert bool((z == 3.0).all()) and bool((src == 5).all())
    s8 = torch.zeros((n, 8), device=DEV, dtype=torch.int32)
    out = f(n, 8, 65)
    with pytest.raises(RuntimeError):
        L.call("moda_merge_rows_fwd", L.ptr(s8), n, 8, 4, 65, L.ptr(f(n, 4, 65)), L.ptr(f(n, 4, 65)), L.ptr(out), L.stream())
    with pytest.raises(RuntimeError):
        R._merge_rows(s8, f(n, 4, 65), f(n, 4, 65))
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ------------------------------------------------------------------------------------------------------------------------ end to end
def test_hierarchical_render_with_two_pdf_entries_per_lane_against_oracle():
    N, S, seed = 6, 256, 52
    models, emb = make_models(seed, 0)
    rays_np = synth.make_rays(seed, N, 0, rays_per_frame=3)
    ref = orc.render_rays(oracle_scene(seed, 0), rays_np, N_samples=S, use_fine=True, perturb=0)
    res = moda_amd.render_rays(models, emb, rays_to_gpu(rays_np), N_samples=S, noise_std=0.0, use_fine=True, perturb=0,
                               opts=make_opts(), img_size=512)
    assert tuple(res["xyz_camera_vis"].shape) == (N, S, 3)
    for k in ("img_coarse", "depth_rnd", "sil_coarse", "xyz_camera_vis"):
        e = rel_err(np_(res[k]), ref[k])
        print(f"hierarchical 128 + 128, {k}: rel {e:.2e}")
        assert e < 1e-4, (k, e)
