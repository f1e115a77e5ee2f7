"""GPU (-m gpu): the bf16-storage backward kernels PER ELEMENT against the float64 / integer references of tests/bwdlayer_numpy.py,
driven through their internal entry points (tests/dev_entries.py) with crafted operands -- moda_bwd256_layer (bwd256_fused.hip),
moda_chain64_bwd, moda_heads64_bwd, moda_pe_ends64_bwd with chain64_reduce_kernel (bwd64_chain.hip) -- and the sign maps of the
bf16-native dW / dX forms of moda_gemm_f32_ex (gemm_bf16.hip).

Every case runs two kinds of data (bwdlayer_numpy's docstring has the construction and the derivation of the bounds):
  exact    small-integer operands (two W variants: at most two signed non-zeros per column, and one-hot): every output is compared
           BIT FOR BIT (array_equal on the patterns) with integer arithmetic, += onto non-zero baselines included.  Two outputs
           keep a bound in this kind: d_xyz, which goes through sine and cosine, and the elements of gW / Tm / g_rgb that `count`
           bf16 subnormals of X reach through a non-zero dZ (a quarter of the columns): count 2^-23 (|baseline| + sum |term|),
           below 0.5 at the largest M, where any dropped or doubled row moves the integer by 2 or more.  Every other element of
           those outputs is bit for bit.
  random   Gaussian operands rounded to bf16, ReLU-shaped activations: fp32 outputs within (n + 1) u sum |term|, bf16 outputs
           inside the interval of the bf16 roundings of truth -+ E, the chains with a running bound.  Nothing is excluded.
Both kinds carry +0.0, -0.0, the positive and the negative bf16 subnormal in X / h / dd / hD on the seam rows: [X > 0] masks both
zeros and passes the positive subnormal unflushed.

Which seam each M crosses (plan constants read from the code):
  bwd256, W = 256   64-sample tiles, streams = min(128, tiles) rounded up to 8, 3 ring stages, the wave halves split a tile at row
                    32.  1, 31, 32, 33, 63, 64, 65: inside one tile / into a second, 7 or 6 of 8 streams empty; 512: 8 tiles, no
                    stream empty; 576: 9 tiles on 16 streams, 7 empty; 8192: one tile on each of 128 streams; 8257: a second tile
                    on stream 0 and a 1-row tile on stream 1; 24576: 3 tiles per stream, the ring's depth; 24641: a fourth tile
                    (the first slot reuse), ragged on stream 1; 32903: five tiles on the first streams, a 7-row tail.
  bwd256, W = 128   streams = min(256, tiles), 4 ring stages.  1, 33, 64, 65; 16384: one tile on each of 256 streams; 16449: a
                    second tile, a 1-row tail; 65536: 4 tiles per stream, the ring's depth; 65601: a fifth tile, the first reuse.
  chain64           128-row tiles, workgroups = min(tiles, 512), the reduce sums partials four at a time in four phases.
                    1 .. 128: one workgroup; 129, 257, 512, 513, 893: 2, 3, 4, 5, 7 workgroups; 65536: 512 workgroups of one
                    tile; 65665: two tiles on the first workgroups, a last tile of 1 row.
  heads64, pe_ends  the same tiles and reduce: 1, 33, 127, 128, 129, 513, 893, 65665; n_out in 1, 16, 25, 32; n_freq 10 and 6 with
                    a window of entries 1, in between and 0.
  sign maps         plan_dw_splits: the 64 x 64 tile plan (R, N <= 64: 4 engines, splits = k-tiles / 8) and the 128 x 128 plan
                    (2 engines, splits = k-tiles / 4, at most 256 / tiles); K = 1, 127, 129 (1 split, ragged), 513 (2 splits on the
                    big plan), 1025 (2 on the small), 8257 (16 small / 32 or more big); N in 32, 64, 128, 256, ld_bits N / 8 and more.
Around the outputs: gb NULL; gW as the skip layer's block at an offset of 63 floats in a wider matrix (the columns around it
bit-untouched); dX / dh / d_xyz pre-filled with NaN patterns with a guard behind them (every element of rows < M written, nothing
else changes); `part` of exactly moda_chain64_part_floats(M) floats with a guard; ld = W + 8 for bwd256 in a test of its own; rows
>= n_out of g_rgb / g_brgb and column 63 of the PE blocks untouched; the map's bytes outside rows < K, columns < N still 0xAA.
Two runs: dX / dh bit-identical; the chains (no atomics: plain stores of partial tiles, one reduce) bit-identical in every
output of both kinds; bwd256's atomics make gW / gb order-dependent in the random kind, bit-identical in the exact kind.

tests/test_bwdlayer_oracle.py pins the references to float64 autograd, asserts the exactness conditions of every case here and
shows that an fp32 model of each kernel's tile order passes, and fails with each of eight planted faults.

No test here exposed a kernel or wrapper bug.  Measured on an MI355X, worst |got - truth| / bound over every case (for a bf16
output |got - truth| / (E + half a bf16 step)):
  bwd256 W = 256     gW 1.00, gb 1.00 (both at M = 1, where the bound is the one rounding of the += and is met exactly; 0.12 and
                     less from M = 33 on), dX 0.99
  bwd256 W = 128     gW 1.00, gb 0.96 (M = 1), dX 0.99
  chain64            gW0..3 1.00, gb1..3 0.99 (M = 1), dh 1.00
  heads64            g_rgb 1.00, g_brgb 0.95, Tm 0.99, svec 0.82 (M = 1), dh 1.00
  pe_ends64          gWa 1.00, gWb 1.00, gb_b 0.98 (M = 1), d_xyz 0.16
  sign maps          gW 1.00, gb 0.99 (K = 1), dX 1.00
  exact kind         every bit-for-bit comparison equal.  The elements a subnormal reaches: some deviate by one fp32 step at
                     small M (W = 256, M = 32: 0.035 of the bound with the sparse W, 0.051 one-hot; M = 64 one-hot: 0.012), none
                     at M = 32903, W = 128 / M = 65601 or chain64 / M = 65665.
  the subnormal      test_mfma_accumulation_of_an_integer_and_a_subnormal_product returns 0x41500000 = 13 exactly for -2^-131 and
                     for +2^-131 in all three placements: two terms alone do not show the deviation.  It shows in the full cases:
                     with 32 rows of integer products summing to 12, a baseline of 1 and one product (-4) 2^-133 the kernel
                     returned 0x414FFFFF = 13 - 2^-20, the same in two runs; every deviation seen was one step downwards.  Which
                     combination of terms inside the instruction produces it is not isolated; the bound does not depend on it.
The module's fixture prints the worst figures (pytest -s).  The whole file (117 tests) takes 24 s, the longest test 2.6 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import bwdlayer_numpy as B

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from moda_amd import _lib as L
    from gpu_helpers import DEV
    import dev_entries

GUARD = 4096
SENTINEL = np.float32(-7777.25)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _worst_figures():
    """After the module's tests: the worst |got - truth| / bound per (entry, output) over the tests that ran (pytest -s)."""
    WORST.clear()
    yield
    for (entry, name), v in sorted(WORST.items()):
        print(f"  worst {entry} {name}: {v:.3g}")


def up16(bits, ld=None, guard=GUARD):
    """A bf16 operand on the device: rows at `ld`, pad columns and the guard behind the last row hold NaN patterns."""
    M, C = bits.shape
    ld = ld or C
    buf = np.full(M * ld + guard, B.NAN_BITS, np.uint16)
    buf[:M * ld].reshape(M, ld)[:, :C] = bits
    return torch.from_numpy(buf.view(np.int16)).to(DEV)


def down16(t, M, ld, C):
    """(the (M, C) patterns, True when pad columns and guard still hold the NaN pattern)."""
    buf = t.cpu().numpy().view(np.uint16)
    body = buf[:M * ld].reshape(M, ld)
    return body[:, :C].copy(), bool((body[:, C:] == B.NAN_BITS).all() and (buf[M * ld:] == B.NAN_BITS).all())


def up32(block, ld=None, off=0, guard=GUARD):
    """An fp32 += output: the baseline block at column offset `off` of a matrix of SENTINEL with leading dimension ld."""
    block = np.atleast_2d(np.asarray(block, np.float32))
    R, C = block.shape
    ld = ld or C
    buf = np.full(R * ld + guard, SENTINEL, np.float32)
    buf[:R * ld].reshape(R, ld)[:, off:off + C] = block
    return torch.from_numpy(buf).to(DEV)


def down32(t, R, C, ld=None, off=0):
    """(the block, True when everything around it is bit-untouched)."""
    ld = ld or C
    buf = t.cpu().numpy()
    body = buf[:R * ld].reshape(R, ld)
    around = np.ones(body.shape, bool)
    around[:, off:off + C] = False
    ok = (B.f32_bits(body[around]) == B.f32_bits(SENTINEL)).all() and (B.f32_bits(buf[R * ld:]) == B.f32_bits(SENTINEL)).all()
    return body[:, off:off + C].copy(), bool(ok)


def fptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def host_ptrs(ps):
    return (ctypes.c_void_p * len(ps))(*[p.value if isinstance(p, ctypes.c_void_p) else p for p in ps])


def judge(tag, ref, got):
    res = B.compare(ref, got, tag)
    for name, (fig, ok) in res.items():
        if ref[name][1] is not None:
            key = (tag.split()[0], name)
            WORST[key] = max(WORST.get(key, 0.0), fig)
    bad = [k for k, v in res.items() if not v[1]]
    assert not bad, (tag, bad, {k: res[k][0] for k in bad})


def same_bits(a, b, names):
    for n in names:
        x, y = a[n], b[n]
        if x.dtype != np.uint16:
            x, y = B.f32_bits(x), B.f32_bits(y)
        assert np.array_equal(x, y), n


def variants(make, *args):
    """The three data sets of a case: (tag, case)."""
    return [("exact/sparse", make("exact", "sparse", *args)), ("exact/onehot", make("exact", "onehot", *args)),
            ("random", make("random", "sparse", *args))]


# ---- moda_bwd256_layer -----------------------------------------------------------------------------------------------------------
def run_bwd256(c, ld=None, with_gb=True, ldg=None, goff=0):
    W, M = c["W"], c["M"]
    ld = ld or W
    fn = dev_entries.entries()["moda_bwd256_layer"]
    dz, x, w = up16(c["dz"], ld), up16(c["x"], ld), up16(c["w"])
    dx = up16(np.full((M, 0), 0, np.uint16), ld)                  # all NaN patterns
    gW, gb = up32(c["gW0"], ldg, goff), up32(c["gb0"])
    rc = fn(W, dz.data_ptr(), ld, x.data_ptr(), ld, w.data_ptr(), W, dx.data_ptr(), ld, fptr(gW, goff), ldg or W,
            fptr(gb) if with_gb else None, M, L.stream())
    assert rc == 0
    torch.cuda.synchronize()
    out = {}
    buf = dx.cpu().numpy().view(np.uint16)
    body = buf[:M * ld].reshape(M, ld)
    out["dX"] = body[:, :W].copy()
    assert (body[:, W:] == B.NAN_BITS).all() and (buf[M * ld:] == B.NAN_BITS).all(), "dX pad columns / guard written"
    out["gW"], ok = down32(gW, W, W, ldg, goff)
    assert ok, "gW: written outside its block"
    g, ok = down32(gb, 1, W)
    assert ok
    if with_gb:
        out["gb"] = g[0]
    else:
        assert np.array_equal(B.f32_bits(g[0]), B.f32_bits(c["gb0"]))
    return out


@pytest.mark.parametrize("W,M", [(256, m) for m in B.M_256] + [(128, m) for m in B.M_128])
def test_bwd256_layer_per_element(W, M):
    for tag, c in variants(B.make_layer, M, W):
        ref = B.ref_layer(c)
        got = run_bwd256(c)
        judge(f"bwd256/{W} M={M} {tag}", ref, got)
        again = run_bwd256(c)
        same_bits(got, again, ("dX", "gW", "gb") if c["kind"] == "exact" else ("dX",))


@pytest.mark.parametrize("row_int,row_sub", [(0, 1), (0, 16), (16, 0)])
def test_mfma_accumulation_of_an_integer_and_a_subnormal_product(row_int, row_sub):
    """The smallest form of the sums for which an element of gW that a bf16 subnormal of X reaches carries a bound in the exact kind.
    moda_bwd256_layer, W = 128, M = 17, W and every other operand element zero, gW's baseline 1 everywhere:
        dZ[row_int][0] = 4, dZ[row_int][1] = 4, X[row_int][33] = 3           12 into gW[0][33] and gW[1][33]
        dZ[row_sub][0] = -4, dZ[row_sub][1] = 4, X[row_sub][33] = 0x0001     -2^-131 into gW[0][33], +2^-131 into gW[1][33]
    Both sums are 13 rounded to nearest.  They are registers 0 and 1 of accumulator accw[0] in lane 1 of wave 5 (i-block 1) of
    workgroup 0; rows 0 .. 15 are the k of the tile's first v_mfma_f32_32x32x16_bf16, row 16 is k = 0 of the second, which
    accumulates onto the first's result: (0, 1) puts both terms into one instruction, (0, 16) adds the subnormal product onto
    the integer, (16, 0) the integer onto the subnormal product.  The patterns are printed and recorded in the module docstring
    (all three return 13 exactly: the deviation of the full cases needs more terms); the assertion is the bound every such
    element has."""
    dz, x = np.zeros((17, 128)), np.zeros((17, 128), np.uint16)
    dz[row_int, :2], dz[row_sub, :2] = 4, (-4, 4)
    x[row_int, 33], x[row_sub, 33] = 0x4040, 0x0001          # 3.0 and the smallest positive subnormal
    c = dict(kind="exact", M=17, W=128, dz=B.bf16_bits(dz), x=x, w=np.zeros((128, 128), np.uint16), gW0=np.ones((128, 128), np.float32),
             gb0=np.ones(128, np.float32))
    ref = B.ref_layer(c)
    got = run_bwd256(c)
    pats = [hex(int(B.f32_bits(got["gW"][o, 33]).ravel()[0])) for o in (0, 1)]
    print(f"  rows {row_int}, {row_sub}: 1 + (12 - 2^-131) = {pats[0]}, 1 + (12 + 2^-131) = {pats[1]}   (13.0 = 0x41500000)")
    assert ref["gW"][1][0, 33] == ref["gW"][1][1, 33] == 2.0 ** -23 * 13 and (ref["gW"][1] > 0).sum() == 2
    judge("mfma integer+subnormal", ref, got)




@pytest.mark.parametrize("W", [256, 128])
@pytest.mark.parametrize("M", [65, 8257])
def test_bwd256_null_bias_and_the_skip_layers_block(W, M):
    for tag, c in variants(B.make_layer, M, W):
        ref = B.ref_layer(c)
        for ldg in (63 + W, 63 + 128 + W):
            got = run_bwd256(c, with_gb=False, ldg=ldg, goff=63)
            judge(f"bwd256/{W} M={M} ldg={ldg} gb=NULL {tag}", ref, got)


@pytest.mark.parametrize("W", [256, 128])
@pytest.mark.parametrize("M", [65, 8257])
def test_bwd256_leading_dimensions_wider_than_the_layer(W, M):
    """ldz = ldx = ldo = W + 8 (the entry accepts it; production passes W): the pad columns of dX stay untouched."""
    for tag, c in variants(B.make_layer, M, W):
        judge(f"bwd256/{W} M={M} ld={W + 8} {tag}", B.ref_layer(c), run_bwd256(c, ld=W + 8))


# ---- the 64-wide chains ----------------------------------------------------------------------------------------------------------
def part_buffer(M):
    n = dev_entries.entries()["moda_chain64_part_floats"](M)
    tiles = (M + 127) // 128
    assert n == min(tiles, 512) * 4 * (64 * 64 + 64)
    return torch.full((n + GUARD,), float(SENTINEL), device=DEV), n


def part_guard_ok(part, n):
    return bool((B.f32_bits(part[n:].cpu().numpy()) == B.f32_bits(SENTINEL)).all())


def run_chain(c, skip_block):
    """skip_block: layer j = 0 as the skip layer -- gb[0] NULL, gW[0] at an offset of 63 floats in rows of 255."""
    M = c["M"]
    fn = dev_entries.entries()["moda_chain64_bwd"]
    dh_in, hs, ws = up16(c["dh"]), [up16(h) for h in c["h"]], [up16(w) for w in c["w"]]
    dh_out = up16(np.full((M, 0), 0, np.uint16), 64)
    ldw = [255 if (skip_block and j == 0) else 64 for j in range(4)]
    off = [63 if (skip_block and j == 0) else 0 for j in range(4)]
    gW = [up32(c["gW0"][j], ldw[j], off[j]) for j in range(4)]
    gb = [up32(c["gb0"][j]) for j in range(4)]
    part, n = part_buffer(M)
    rc = fn(dh_in.data_ptr(), 64, host_ptrs([h.data_ptr() for h in hs]), 64, host_ptrs([w.data_ptr() for w in ws]), dh_out.data_ptr(), 64,
            host_ptrs([fptr(gW[j], off[j]) for j in range(4)]), (ctypes.c_longlong * 4)(*ldw),
            host_ptrs([None if (skip_block and j == 0) else fptr(gb[j]) for j in range(4)]), 4, M, fptr(part), L.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert part_guard_ok(part, n), "part: written past moda_chain64_part_floats(M)"
    out = {}
    out["dh"], ok = down16(dh_out, M, 64, 64)
    assert ok
    for j in range(4):
        out[f"gW{j}"], ok = down32(gW[j], 64, 64, ldw[j], off[j])
        assert ok, f"gW{j}: written outside its block"
        g, ok = down32(gb[j], 1, 64)
        assert ok
        if skip_block and j == 0:
            assert np.array_equal(B.f32_bits(g[0]), B.f32_bits(c["gb0"][j]))
        else:
            out[f"gb{j}"] = g[0]
    return out


@pytest.mark.parametrize("M", B.M_CHAIN)
def test_chain64_per_element(M):
    for (tag, c), skip_block in zip(variants(B.make_chain, M), (False, True, True)):
        ref = B.ref_chain(c)
        got = run_chain(c, skip_block)
        judge(f"chain64 M={M} skip_block={skip_block} {tag}", ref, got)
        same_bits(got, run_chain(c, skip_block), got.keys())        # no atomics: every output repeats bit for bit


def run_heads(c):
    M, n_out = c["M"], c["n_out"]
    fn = dev_entries.entries()["moda_heads64_bwd"]
    dz, dd, hD, wrgb, wext = (up16(c[k]) for k in ("dz", "dd", "hD", "wrgb", "wext"))
    dh = up16(np.full((M, 0), 0, np.uint16), 64)
    g_rgb, g_brgb, Tm, svec = up32(c["g_rgb0"]), up32(c["g_brgb0"]), up32(c["Tm0"]), up32(c["svec0"])
    part, n = part_buffer(M)
    rc = fn(dz.data_ptr(), 32, dd.data_ptr(), 32, hD.data_ptr(), 64, wrgb.data_ptr(), wext.data_ptr(), dh.data_ptr(), 64, fptr(g_rgb), 32,
            fptr(g_brgb), n_out, fptr(Tm), fptr(svec), M, fptr(part), L.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert part_guard_ok(part, n)
    out = {}
    out["dh"], ok = down16(dh, M, 64, 64)
    assert ok
    for name, t, R, C in (("g_rgb", g_rgb, 32, 32), ("g_brgb", g_brgb, 1, 32), ("Tm", Tm, 32, 64), ("svec", svec, 1, 32)):
        g, ok = down32(t, R, C)
        assert ok, name
        out[name] = g if R > 1 else g[0]
    assert np.array_equal(B.f32_bits(out["g_rgb"][n_out:]), B.f32_bits(c["g_rgb0"][n_out:])), "g_rgb rows >= n_out touched"
    assert np.array_equal(B.f32_bits(out["g_brgb"][n_out:]), B.f32_bits(c["g_brgb0"][n_out:])), "g_brgb entries >= n_out touched"
    return out


@pytest.mark.parametrize("n_out", B.N_OUT)
@pytest.mark.parametrize("M", B.M_HEADS)
def test_heads64_per_element(M, n_out):
    for tag, c in variants(B.make_heads, M, n_out):
        got = run_heads(c)
        judge(f"heads64 M={M} n_out={n_out} {tag}", B.ref_heads(c), got)
        same_bits(got, run_heads(c), got.keys())


def run_pe(c, with_gb):
    M = c["M"]
    fn = dev_entries.entries()["moda_pe_ends64_bwd"]
    dha, dhb, pe, wa, wb = (up16(c[k]) for k in ("dha", "dhb", "pe", "wa", "wb"))
    xyz = torch.from_numpy(c["xyz"]).to(DEV)
    d_xyz = torch.from_numpy(np.full(M * 3 + GUARD, np.nan, np.float32)).to(DEV)
    gWa, gWb, gbb = up32(c["gWa0"], 255, 1), up32(c["gWb0"], 191, 65), up32(c["gbb0"])
    part, n = part_buffer(M)
    win = (ctypes.c_float * len(c["win"]))(*[float(v) for v in c["win"]])
    rc = fn(dha.data_ptr(), dhb.data_ptr(), 64, pe.data_ptr(), 64, wa.data_ptr(), wb.data_ptr(), xyz.data_ptr(), c["n_freq"],
            ctypes.cast(win, ctypes.c_void_p), fptr(gWa, 1), 255, fptr(gWb, 65), 191, fptr(gbb) if with_gb else None, fptr(d_xyz), M,
            fptr(part), L.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert part_guard_ok(part, n)
    out = {}
    d = d_xyz.cpu().numpy()
    out["d_xyz"] = d[:M * 3].reshape(M, 3).copy()
    assert np.isfinite(out["d_xyz"]).all() and np.isnan(d[M * 3:]).all(), "d_xyz: an element unwritten, or the guard written"
    out["gWa"], ok = down32(gWa, 64, 63, 255, 1)        # `around` includes column 63 of the block
    assert ok, "gWa: written outside its 64 x 63 block"
    out["gWb"], ok = down32(gWb, 64, 63, 191, 65)
    assert ok, "gWb: written outside its 64 x 63 block"
    g, ok = down32(gbb, 1, 64)
    assert ok
    if with_gb:
        out["gb_b"] = g[0]
    else:
        assert np.array_equal(B.f32_bits(g[0]), B.f32_bits(c["gbb0"]))
    return out


@pytest.mark.parametrize("n_freq,alpha", B.PE_WINDOWS)
@pytest.mark.parametrize("M", B.M_HEADS)
def test_pe_ends64_per_element(M, n_freq, alpha):
    w = B.window(n_freq, alpha)
    assert (w == 1).any() and (w == 0).any() and ((w > 0) & (w < 1)).any()
    for kind, with_gb in (("exact", True), ("random", False), ("random", True)):
        c = B.make_pe(kind, M, n_freq, alpha)
        got = run_pe(c, with_gb)
        judge(f"pe_ends64 M={M} n_freq={n_freq} gb_b={with_gb} {kind}", B.ref_pe(c), got)
        same_bits(got, run_pe(c, with_gb), got.keys())


# ---- the sign maps of the bf16-native dW / dX forms --------------------------------------------------------------------------------
BF, FA, FB, FC, FM = 1, 2, 4, 8, 16


def gemm(**kw):
    d = dict(A=None, sam=0, sak=0, A2=None, sam2=0, K1=0, B=None, sbk=0, sbn=1, C=None, ldc=0, M=0, N=0, K=0, bias=None, rowbias=None,
             ld_rowbias=0, rows_per_bias=1, mask_src=None, ld_mask=0, act=0, accumulate=0, split_k=1, reserved=0, a_sum=None,
             mask_bits=None, ld_bits=0)
    d.update(kw)
    L.call("moda_gemm_f32_ex", ctypes.byref(L.GemmDesc(**d)), L.stream())


@pytest.mark.parametrize("R,N", B.RN_MAPS)
@pytest.mark.parametrize("K", B.K_MAPS)
def test_sign_maps_of_the_bf16_native_gemm_forms(K, R, N):
    for tag, c in variants(B.make_rect, K, R, N):
        ref = B.ref_layer(c)
        want_map = B.ref_signmap(c["x"])
        assert not (want_map == 0xAA).all()
        for ld_bits in (N // 8, N // 8 + 3):
            # dW form: gW += dZ^T X, db += 1^T dZ, the map of [X > 0] written
            dz, x, w = up16(c["dz"]), up16(c["x"]), up16(c["w"])
            gW, gb = up32(c["gW0"]), up32(c["gb0"])
            bits = torch.full((K * ld_bits + GUARD,), 0xAA, dtype=torch.uint8, device=DEV)
            gemm(A=dz.data_ptr(), sam=1, sak=R, B=x.data_ptr(), sbk=N, C=gW.data_ptr(), ldc=N, M=R, N=N, K=K, accumulate=1,
                 reserved=BF | FA | FB, a_sum=gb.data_ptr(), mask_bits=bits.data_ptr(), ld_bits=ld_bits)
            torch.cuda.synchronize()
            m = bits.cpu().numpy()
            body = m[:K * ld_bits].reshape(K, ld_bits)
            assert not (body == 0xAA).all(), "the map was not written: the call fell to the generic kernel"
            assert np.array_equal(body[:, :N // 8], want_map), "sign map != [B > 0]"
            assert (body[:, N // 8:] == 0xAA).all() and (m[K * ld_bits:] == 0xAA).all(), "map bytes outside rows < K, columns < N written"
            got = {}
            got["gW"], ok = down32(gW, R, N)
            assert ok
            g, ok = down32(gb, 1, R)
            assert ok
            got["gb"] = g[0]
            # dX form reading the map just written, and the same call with the bf16 mask source
            outs = []
            for use_bits in (True, False):
                dx = up16(np.full((K, 0), 0, np.uint16), N)
                kw = dict(mask_bits=bits.data_ptr(), ld_bits=ld_bits, reserved=BF | FA | FB | FC) if use_bits else \
                    dict(mask_src=x.data_ptr(), ld_mask=N, reserved=BF | FA | FB | FC | FM)
                gemm(A=dz.data_ptr(), sam=R, sak=1, B=w.data_ptr(), sbk=N, C=dx.data_ptr(), ldc=N, M=K, N=N, K=R, **kw)
                torch.cuda.synchronize()
                o, ok = down16(dx, K, N, N)
                assert ok
                outs.append(o)
            assert np.array_equal(outs[0], outs[1]), "dX through the map != dX through mask_src"
            got["dX"] = outs[0]
            judge(f"signmap K={K} R={R} N={N} ld_bits={ld_bits} {tag}", ref, got)
