"""Float64 references, per-element bounds, fp32 tile-order models and the case builders of the bf16-storage backward kernels
(csrc/bwd256_fused.hip moda_bwd256_layer; csrc/bwd64_chain.hip moda_chain64_bwd, moda_heads64_bwd, moda_pe_ends64_bwd and
chain64_reduce_kernel; the sign maps of csrc/gemm_bf16.hip), written from the formulas in those files' header comments.  Nothing
here imports the package.  u = U = 2^-24.

  layer     gW += dZ^T X     gb += 1^T dZ     dX = bf16((dZ W) (.) [X > 0])          dZ (M, O), X (M, I), W (O, I) = [o][i]
  chain64   four layers; dh is rounded to bf16 between layers and db_l is summed from the rounded dh_l
  heads64   layer (dz_rgb, dd, Wrgb) -> g_rgb, g_brgb, dzd;  layer (dzd, hD, Wext) -> Tm, svec, dh
  pe_ends   gWa[:, :63] += dh_a^T PE, gWb[:, :63] += dh_b^T PE, gb_b += 1^T dh_b, d_pe = dh_a Wa + dh_b Wb (fp32, never stored),
            d_xyz[m, c] = d_pe[m, c] + sum_k w_k 2^k (cos(2^k x) d_pe[m, 3 + 6k + c] - sin(2^k x) d_pe[m, 6 + 6k + c])

Every reference returns name -> (truth, bound), float64 both; bound None means every element is an exact statement, and so does
an element with bound 0.  Nothing is excluded anywhere.  The bounds are those of a sum of exact bf16 x bf16 products in ANY
order -- partial tiles, the reduce and atomics included -- each addition costing at most u times the magnitude of its result:
  fp32 output summing n products onto a baseline   |got - truth| <= n u (|baseline| + sum |term|): n + 1 terms take n additions;
                                                   n = M for gW / gb / Tm / svec / g_rgb
  bf16 output (dX, dh, dzd)                        truth and E are those of the fp32 value BEFORE the rounding, E = K u sum |term|,
                                                   K = the products per element (the layer's O); got must lie between the bf16
                                                   roundings of truth - E and truth + E (in_bf16_interval): a tie may round either
                                                   way, nothing else passes.  Masked elements have truth 0 and E 0: exactly 0.
  through a chain                                  e_l = the bound of |dh_l(kernel) - dh_l(reference)| after rounding = the larger
                                                   distance from the reference's rounded value to the two ends of that interval
                                                   (0 at the chain's input); it enters layer l - 1 as e |W| (masked) next to that
                                                   layer's own E, gW as sum_m e |h| and gb as sum_m e; |dh| + e stands for |dh| in
                                                   every sum of magnitudes.
  d_xyz                                            n u (sum_j |coef_j| A_j) + S: A_j = sum |dh||w| of d_pe column j, coef_j the
                                                   float64 factor of that column, n = 128 + 2 n_freq + 1 (the products of d_pe plus
                                                   the terms of the coordinate); S = sum_k w_k 2^k EPS_SINCOS (|g_sin| + |g_cos|):
                                                   the kernel's sincos_rr is a polynomial with a stated absolute error of 1.3e-7
                                                   (moda_dev.h); sine and cosine of the truth are float64 of the same fp32 xyz.
u per addition is the figure of round-to-nearest.  The atomics, the reduce and every VALU addition round to nearest; the
accumulation inside v_mfma_f32_32x32x16_bf16 does not always (below), and an addition that rounds one way costs up to 2 u.  The
bounds keep u: they are the stricter statement, a worst case over n additions all erring the same way, and the kernels sit far
inside them from M = 33 on (figures in tests/test_gpu_bwdlayer.py).  At M = 1 the one addition is the atomic's or the
reduce's, which rounds to nearest, and the bound is met with nothing to spare.

The EXACT kind: operands are small integers held as bf16 (even dZ, W in {-1, 0, 1} with at most two non-zeros per column -- |dh|
at most doubles per chained layer -- or exactly one: the signed one-hot variant; PE rows k / 128), baselines odd integers (odd /
128 for the PE blocks).  Every product is exact in fp32 and, as long as |baseline| + sum |term| < 2^24 units, so is every sum in
any order: each output equals integer arithmetic bit for bit.  assert_exact states these conditions on the reference of every
case: integer truths, the magnitude sums below 2^24 units, bf16-stored results integers <= 256.

One class of elements is no integer sum.  The special mask values below put +-2^-133 into X, so an element of gW / Tm / g_rgb
that such a value reaches through a non-zero dZ is an integer plus `count` terms of at most 2^-125 each (count = the number of
such rows, layer_ref; a quarter of the columns have count > 0).  Rounded to nearest the sum is still the integer, but the
accumulation of v_mfma_f32_32x32x16_bf16 has been seen to return the next fp32 BELOW it (13 - 2^-20 for 12 + (-4) 2^-133 on a
baseline of 1; tests/test_gpu_bwdlayer.py records when it does and that two terms alone do not show it).  Each such term moves
the running sum by at most one fp32 step of its magnitude, at most 2^-23 (|baseline| + sum |term|), and the steps neither grow
nor multiply afterwards: an integer less one step plus an integer is again an integer less one step of the larger magnitude.
These elements carry the bound count 2^-23 (|baseline| + sum |term|) in the exact kind, which assert_exact
holds below 1 for every case, while a dropped, doubled or misplaced row moves the integer by 2 or more (dZ is even); every other
element of those outputs has bound 0.  gb, dX and dh never see the values of X and are exact throughout.

Special mask values go into X / h / dd / hD of both kinds on the rows of seam_rows (tile seams and the ends of M), four columns
in sixteen (low and high halves of a 32-bit pair by the row's parity): +0.0, -0.0, the smallest positive bf16 subnormal (0x0001)
and the largest negative (0x8001).  The contract is [X > 0] (moda_hip.h: bit = [element > 0]): both zeros and the negative
subnormal are masked, the positive subnormal passes.

The fp32 models (model_bwd256, model_chain, model_pe_ends, model_signmap) walk the tiles in each kernel's order -- streams /
workgroups, tiles p, p + P, ..., per-workgroup accumulators, db by row groups, the four phases of chain64_reduce_kernel with its
4-way unrolled loop and remainder -- and carry the FAULTS switches tests/test_bwdlayer_oracle.py plants."""
import numpy as np

U = 2.0 ** -24
EPS_SINCOS = 1.3e-7                      # sincos_rr, moda_dev.h: "absolute error <= 1.3e-7"
SPECIALS = np.array([0x0000, 0x8000, 0x0001, 0x8001], np.uint16)
NAN_BITS = 0x7FC1                        # the pre-fill of bf16 outputs
LIMIT = 2.0 ** 24

M_256 = (1, 31, 32, 33, 63, 64, 65, 512, 576, 8192, 8257, 24576, 24641, 32903)
M_128 = (1, 33, 64, 65, 16384, 16449, 65536, 65601)
M_CHAIN = (1, 33, 65, 127, 128, 129, 257, 512, 513, 893, 65536, 65665)
M_HEADS = (1, 33, 127, 128, 129, 513, 893, 65665)
N_OUT = (1, 16, 25, 32)
PE_WINDOWS = ((10, 6.3), (6, 3.4))       # (n_freq, annealing position): window entries 1, in between and 0
K_MAPS = (1, 127, 129, 513, 1025, 8257)  # sign maps: rows of B
RN_MAPS = ((64, 32), (64, 64), (128, 128), (256, 256))      # (columns of dZ, columns of B)
KINDS = ("exact", "random")
FAULTS = ("short_row", "skip_ring_tile", "db_half", "no_remainder", "mask_ge", "mask_neighbour", "flush_subnormal",
          "bits_wrong_rows")


# ---- bf16 ----------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """Round to nearest even to bf16 (through fp32); the uint16 patterns."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(bits, dtype=np.float64):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(dtype)


def bf16_round(x):
    return bf16_val(bf16_bits(x))


def f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def in_bf16_interval(got_bits, truth, E):
    """got (bf16 patterns) between the bf16 roundings of truth - E and truth + E, per element."""
    g = bf16_val(got_bits)
    return (g >= bf16_round(truth - E)) & (g <= bf16_round(truth + E))


def fraction_f32(got, truth, bound):
    """(worst |got - truth| / bound over bound > 0, every element within its bound: bound 0 means equal)."""
    err = np.abs(np.asarray(got, np.float64) - truth)
    pos = bound > 0
    frac = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    return frac, bool((err <= bound).all())


def bf16_half_step(v):
    """Half the distance between neighbouring bf16 values at v (float64)."""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64) * 2.0 ** 15


def fraction_bf16(got_bits, truth, E):
    """(worst |got - truth| / (E + half a bf16 step at truth), every element inside its interval).  The figure is a distance in
    units of what the fp32 bound and one rounding allow together; the assertion is the interval."""
    err = np.abs(bf16_val(got_bits) - truth)
    frac = float((err / (E + bf16_half_step(bf16_round(truth)))).max()) if err.size else 0.0
    return frac, bool(in_bf16_interval(got_bits, truth, E).all())


# ---- data ----------------------------------------------------------------------------------------------------------------------
def seam_rows(M, tile):
    last = (M - 1) // tile * tile
    c = {0, 1, 31, 32, 33, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, last - 1, last, M - 2, M - 1}
    return sorted(r for r in c if 0 <= r < M)


def plant_specials(xbits, tile):
    """Columns 1, 5, 9, 13 (mod 16) of an even seam row, 2, 6, 10, 14 of an odd one: +0.0, -0.0, +subnormal, -subnormal."""
    j = np.arange(xbits.shape[1])
    for r in seam_rows(xbits.shape[0], tile):
        ph = (j - (r & 1)) % 16
        xbits[r, ph % 4 == 1] = SPECIALS[ph[ph % 4 == 1] // 4]
    return xbits


def activations(rng, kind, M, I, tile):
    """ReLU-shaped, about half zeros, with the special values on the seam rows."""
    if kind == "exact":
        v = rng.integers(1, 4, (M, I)) * (rng.random((M, I)) < 0.5)
    else:
        v = np.maximum(rng.standard_normal((M, I)), 0.0)
    return plant_specials(bf16_bits(v), tile)


def gradients(rng, kind, M, O, amp=4):
    return bf16_bits(2 * rng.integers(-amp, amp + 1, (M, O)) if kind == "exact" else rng.standard_normal((M, O)))


def weights(rng, kind, variant, O, I, rows=None):
    """[o][i]; rows >= `rows` zero.  exact: signed, at most two non-zeros per column ('sparse') or exactly one ('onehot': for
    O == I a signed permutation)."""
    rows = O if rows is None else rows
    w = np.zeros((O, I))
    if kind == "exact":
        i = np.arange(I)
        perm = rng.permutation(rows)
        r1 = perm[i % rows]
        w[r1, i] = rng.choice([-1.0, 1.0], I)
        if variant == "sparse" and rows > 1:
            r2 = (r1 + 1 + rng.integers(0, rows - 1, I)) % rows
            w[r2, i] = rng.choice([-1.0, 1.0], I)
    else:
        w[:rows] = rng.standard_normal((rows, I)) / np.sqrt(O)
    return bf16_bits(w)


def baseline(rng, kind, shape, unit=1.0):
    """Non-zero start of a += output: odd integers (times unit) in the exact kind."""
    if kind == "exact":
        return ((2 * rng.integers(-5, 5, shape) + 1) * unit).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def make_layer(kind, variant, M, W, seed=0):
    rng = np.random.default_rng([seed, M, W, KINDS.index(kind), variant == "onehot"])
    return dict(kind=kind, M=M, W=W, dz=gradients(rng, kind, M, W), x=activations(rng, kind, M, W, 64),
                w=weights(rng, kind, variant, W, W), gW0=baseline(rng, kind, (W, W)), gb0=baseline(rng, kind, (W,)))


def make_rect(kind, variant, K, R, N, seed=11):
    """One layer with dZ (K, R), X (K, N), W (R, N): the operands of the bf16-native dW / dX forms and their sign maps."""
    rng = np.random.default_rng([seed, K, R, N, KINDS.index(kind), variant == "onehot"])
    return dict(kind=kind, M=K, dz=gradients(rng, kind, K, R), x=activations(rng, kind, K, N, 64),
                w=weights(rng, kind, variant, R, N), gW0=baseline(rng, kind, (R, N)), gb0=baseline(rng, kind, (R,)))


def make_chain(kind, variant, M, seed=0):
    rng = np.random.default_rng([seed, M, 64, KINDS.index(kind), variant == "onehot"])
    return dict(kind=kind, M=M, dh=gradients(rng, kind, M, 64, amp=1), h=[activations(rng, kind, M, 64, 128) for _ in range(4)],
                w=[weights(rng, kind, variant, 64, 64) for _ in range(4)], gW0=[baseline(rng, kind, (64, 64)) for _ in range(4)],
                gb0=[baseline(rng, kind, (64,)) for _ in range(4)])


def make_heads(kind, variant, M, n_out, seed=0):
    rng = np.random.default_rng([seed, M, n_out, KINDS.index(kind), variant == "onehot"])
    dz = gradients(rng, kind, M, 32, amp=2)
    dz[:, n_out:] = 0
    return dict(kind=kind, M=M, n_out=n_out, dz=dz, dd=activations(rng, kind, M, 32, 128), hD=activations(rng, kind, M, 64, 128),
                wrgb=weights(rng, kind, variant, 32, 32, rows=n_out), wext=weights(rng, kind, variant, 32, 64),
                g_rgb0=baseline(rng, kind, (32, 32)), g_brgb0=baseline(rng, kind, (32,)), Tm0=baseline(rng, kind, (32, 64)),
                svec0=baseline(rng, kind, (32,)))


def window(n_freq, alpha):
    """The fp32 window of Embedding (nerf.py:35-75) at annealing position alpha: entries 1, in between, 0."""
    w = np.clip(alpha - np.arange(n_freq), 0.0, 1.0)
    return (0.5 * (1 + np.cos(np.pi * w + np.pi))).astype(np.float32)


def make_pe(kind, M, n_freq, alpha, seed=0):
    rng = np.random.default_rng([seed, M, n_freq, KINDS.index(kind), 7])
    if kind == "exact":
        dha, dhb = (bf16_bits(2 * rng.integers(-1, 2, (M, 64)) * (rng.random((M, 64)) < 0.5)) for _ in range(2))
        pe = bf16_bits(rng.integers(-128, 129, (M, 64)) / 128.0)
        wa, wb = (bf16_bits(rng.integers(-3, 4, (64, 64))) for _ in range(2))
    else:
        dha, dhb = (bf16_bits(rng.standard_normal((M, 64))) for _ in range(2))
        pe = bf16_bits(np.sin(3 * rng.standard_normal((M, 64))))
        wa, wb = (bf16_bits(rng.standard_normal((64, 64)) / 8) for _ in range(2))
    pe[:, 63] = 0
    return dict(kind=kind, M=M, n_freq=n_freq, dha=dha, dhb=dhb, pe=pe, wa=wa, wb=wb,
                xyz=(1.5 * rng.standard_normal((M, 3))).astype(np.float32), win=window(n_freq, alpha),
                gWa0=baseline(rng, kind, (64, 63), 1 / 128), gWb0=baseline(rng, kind, (64, 63), 1 / 128),
                gbb0=baseline(rng, kind, (64,)))


# ---- references ----------------------------------------------------------------------------------------------------------------
def assert_exact(truth, mag, unit=1.0, stored_max=None, tiny_ok=False):
    """The exactness conditions of one output of an exact-kind case: truth a whole number of units (tiny_ok: X's +-2^-133 terms
    may ride on it -- beside a non-zero integer they are below float64's resolution, and the integer part must be non-zero),
    sum of magnitudes below 2^24 units, bf16-stored values at most stored_max."""
    t = np.asarray(truth) / unit
    r = np.rint(t)
    if tiny_ok:
        off = t != r
        assert (np.abs(t - r) < 2.0 ** -100).all() and (r[off] != 0).all()
    else:
        assert (t == r).all()
    assert (np.asarray(mag) / unit < LIMIT).all()
    if stored_max is not None:
        assert (np.abs(r) <= stored_max).all()
    return r * unit


def layer_ref(dz, x, w, gW0, gb0, exact, e=None, unit=1.0):
    """One layer on float64 values.  Returns (outputs, dX rounded to bf16 as float64, the bound e of the next layer's dh)."""
    M, O = dz.shape
    gW0, gb0 = np.asarray(gW0, np.float64), np.asarray(gb0, np.float64)
    adz = np.abs(dz) if e is None else np.abs(dz) + e
    gW, gb, pre = gW0 + dz.T @ x, gb0 + dz.sum(0), dz @ w
    mW, mb, mX = np.abs(gW0) + adz.T @ np.abs(x), np.abs(gb0) + adz.sum(0), adz @ np.abs(w)
    keep = x > 0
    pre = np.where(keep, pre, 0.0) + 0.0
    if exact:
        assert e is None
        gW = assert_exact(gW, mW, unit, tiny_ok=True)
        gb = assert_exact(gb, mb)
        pre = assert_exact(pre, mX, stored_max=256)
        # elements of gW that `count` subnormals of X reach through a non-zero dZ: one fp32 step of the running sum each
        count = (dz != 0).T.astype(np.float64) @ ((x != 0) & (np.abs(x) < 2.0 ** -126)).astype(np.float64)
        bW = count * 2.0 ** -23 * mW
        assert (bW < unit).all()
        return dict(gW=(gW, bW), gb=(gb, None), dX=(pre, None)), pre, None
    bW, bb, E = M * U * mW, M * U * mb, O * U * mX
    if e is not None:
        bW, bb, E = bW + e.T @ np.abs(x), bb + e.sum(0), E + e @ np.abs(w)
    E = np.where(keep, E, 0.0)
    dx = bf16_round(pre)
    e_next = np.maximum(bf16_round(pre + E) - dx, dx - bf16_round(pre - E))
    return dict(gW=(gW, bW), gb=(gb, bb), dX=(pre, E)), dx, e_next


def ref_layer(c):
    return layer_ref(bf16_val(c["dz"]), bf16_val(c["x"]), bf16_val(c["w"]), c["gW0"], c["gb0"], c["kind"] == "exact")[0]


def chain_ref(dh, hs, ws, gW0s, gb0s, exact):
    out, e = {}, None
    for l in range(len(hs)):
        r, dh, e = layer_ref(dh, hs[l], ws[l], gW0s[l], gb0s[l], exact, e)
        out[f"gW{l}"], out[f"gb{l}"], out[f"dX{l}"] = r["gW"], r["gb"], r["dX"]
    return out


def ref_chain(c):
    """gW0..3, gb0..3 and dh (= dX3; dX0..2 are the intermediate dh the kernel keeps in LDS)."""
    out = chain_ref(bf16_val(c["dh"]), [bf16_val(h) for h in c["h"]], [bf16_val(w) for w in c["w"]], c["gW0"], c["gb0"],
                    c["kind"] == "exact")
    out["dh"] = out["dX3"]
    return out


def ref_heads(c):
    """g_rgb (32 x 32: rows >= n_out keep their baseline, the products there being zero), g_brgb, Tm, svec, dh."""
    out = chain_ref(bf16_val(c["dz"]), [bf16_val(c["dd"]), bf16_val(c["hD"])], [bf16_val(c["wrgb"]), bf16_val(c["wext"])],
                    [c["g_rgb0"], c["Tm0"]], [c["g_brgb0"], c["svec0"]], c["kind"] == "exact")
    return dict(g_rgb=out["gW0"], g_brgb=out["gb0"], Tm=out["gW1"], svec=out["gb1"], dh=out["dX1"], dzd=out["dX0"])


def embed_backward(dpe, xyz, win):
    """d_xyz of Embedding's backward, float64: dpe (M, >= 3 + 6 n_freq), xyz (M, 3), win (n_freq)."""
    d = dpe[:, :3].copy()
    for k in range(len(win)):
        f = 2.0 ** k
        d += win[k] * f * (np.cos(f * xyz) * dpe[:, 3 + 6 * k:6 + 6 * k] - np.sin(f * xyz) * dpe[:, 6 + 6 * k:9 + 6 * k])
    return d


def ref_pe(c):
    exact = c["kind"] == "exact"
    M, nf = c["M"], c["n_freq"]
    dha, dhb, pe, wa, wb = (bf16_val(c[k]) for k in ("dha", "dhb", "pe", "wa", "wb"))
    out = {}
    for name, dh, g0 in (("gWa", dha, c["gWa0"]), ("gWb", dhb, c["gWb0"])):
        g0 = np.asarray(g0, np.float64)
        t, mag = g0 + dh.T @ pe[:, :63], np.abs(g0) + np.abs(dh).T @ np.abs(pe[:, :63])
        out[name] = (assert_exact(t, mag, 1 / 128), None) if exact else (t, M * U * mag)
    g0 = np.asarray(c["gbb0"], np.float64)
    t, mag = g0 + dhb.sum(0), np.abs(g0) + np.abs(dhb).sum(0)
    out["gb_b"] = (assert_exact(t, mag), None) if exact else (t, M * U * mag)
    dpe, A = dha @ wa + dhb @ wb, np.abs(dha) @ np.abs(wa) + np.abs(dhb) @ np.abs(wb)
    if exact:
        assert_exact(dpe, A)
    xyz, win = c["xyz"].astype(np.float64), c["win"].astype(np.float64)
    mag, S = A[:, :3].copy(), np.zeros((M, 3))
    for k in range(nf):
        f = 2.0 ** k
        g1, g2 = slice(3 + 6 * k, 6 + 6 * k), slice(6 + 6 * k, 9 + 6 * k)
        mag += win[k] * f * (np.abs(np.cos(f * xyz)) * A[:, g1] + np.abs(np.sin(f * xyz)) * A[:, g2])
        S += win[k] * f * EPS_SINCOS * (np.abs(dpe[:, g1]) + np.abs(dpe[:, g2]))
    out["d_xyz"] = (embed_backward(dpe, xyz, win), (128 + 2 * nf + 1) * U * mag + S)
    return out


def ref_signmap(bbits):
    """[B > 0] packed: bit (n & 7) of byte n >> 3."""
    return np.packbits(bf16_val(bbits) > 0, axis=1, bitorder="little")


# ---- fp32 models in the kernels' tile order, with the planted faults -----------------------------------------------------------
def keep_mask(xbits, fault=None):
    """The kernels' mask of a tile's rows: the 16 bits as a signed integer > 0."""
    s = np.ascontiguousarray(xbits, np.uint16).view(np.int16)
    if fault == "mask_neighbour":
        s = np.roll(s, -1, axis=0)
    if fault == "mask_ge":
        return s >= 0
    if fault == "flush_subnormal":
        return (s > 0) & ((xbits & 0x7F80) != 0)
    return s > 0


def bwd256_plan(W, M):
    """(tiles, streams, ring stages) as b256_launch and Geo<WD> choose them."""
    tiles = (M + 63) // 64
    P = min(128 if W == 256 else 256, tiles)
    if W == 256:
        P = (P + 7) // 8 * 8
    return tiles, P, 3 if W == 256 else 4


def model_bwd256(c, fault=None):
    M, W = c["M"], c["W"]
    tiles, P, nstage = bwd256_plan(W, M)
    dz, x, w = (bf16_val(c[k], np.float32) for k in ("dz", "x", "w"))
    gW, gb = c["gW0"].astype(np.float32).copy(), c["gb0"].astype(np.float32).copy()
    dX = np.full((M, W), NAN_BITS, np.uint16)
    for p in range(min(P, tiles)):
        acc, sdb = np.zeros((W, W), np.float32), np.zeros(W, np.float32)
        for k, t in enumerate(range(p, tiles, P)):
            r0 = t * 64
            nv = min(64, M - r0)
            if fault == "short_row" and nv < 64:
                nv -= 1
            if nv <= 0 or (fault == "skip_ring_tile" and k == nstage):
                continue
            z, xt = dz[r0:r0 + nv], x[r0:r0 + nv]
            acc += z.T @ xt
            sdb += z[:32].sum(0, dtype=np.float32)
            if fault != "db_half":
                sdb += z[32:].sum(0, dtype=np.float32)
            dX[r0:r0 + nv] = bf16_bits(np.where(keep_mask(c["x"][r0:r0 + nv], fault), z @ w, np.float32(0)))
        gW += acc
        gb += sdb
    return dict(gW=gW, gb=gb, dX=dX)


def reduce_partials(part, fault=None):
    """chain64_reduce_kernel: part (nwg, ...) fp32; four phases, each a 4-way unrolled loop and a remainder."""
    nwg = part.shape[0]
    red = []
    for ph in range(4):
        s = [np.zeros(part.shape[1:], np.float32) for _ in range(4)]
        w = ph
        while w + 12 < nwg:
            for q in range(4):
                s[q] = s[q] + part[w + 4 * q]
            w += 16
        while w < nwg and fault != "no_remainder":
            s[0] = s[0] + part[w]
            w += 4
        red.append((s[0] + s[1]) + (s[2] + s[3]))
    return (red[0] + red[1]) + (red[2] + red[3])


def model_chain_generic(M, dh_bits, h_bits, w_bits, gW0s, gb0s, fault=None):
    NL = len(h_bits)
    tiles = (M + 127) // 128
    nwg = min(tiles, 512)
    dh32, ws = bf16_val(dh_bits, np.float32), [bf16_val(w, np.float32) for w in w_bits]
    hs = [bf16_val(h, np.float32) for h in h_bits]
    pW = [np.zeros((nwg,) + ws[l].shape, np.float32) for l in range(NL)]
    pb = [np.zeros((nwg, ws[l].shape[0]), np.float32) for l in range(NL)]
    mids = [np.full((M, ws[l].shape[1]), NAN_BITS, np.uint16) for l in range(NL)]
    for g in range(nwg):
        for t in range(g, tiles, nwg):
            r0 = t * 128
            nv = min(128, M - r0)
            if fault == "short_row" and nv < 128:
                nv -= 1
            if nv <= 0:
                continue
            dh = dh32[r0:r0 + nv]
            for l in range(NL):
                pW[l][g] += dh.T @ hs[l][r0:r0 + nv]
                for rg in range(2 if fault == "db_half" else 4):
                    pb[l][g] += dh[32 * rg:32 * rg + 32].sum(0, dtype=np.float32)
                bits = bf16_bits(np.where(keep_mask(h_bits[l][r0:r0 + nv], fault), dh @ ws[l], np.float32(0)))
                mids[l][r0:r0 + nv] = bits
                dh = bf16_val(bits, np.float32)
    out = {}
    for l in range(NL):
        out[f"gW{l}"] = gW0s[l].astype(np.float32) + reduce_partials(pW[l], fault)
        out[f"gb{l}"] = gb0s[l].astype(np.float32) + reduce_partials(pb[l], fault)
        out[f"dX{l}"] = mids[l]
    return out


def model_chain(c, fault=None):
    out = model_chain_generic(c["M"], c["dh"], c["h"], c["w"], c["gW0"], c["gb0"], fault)
    out["dh"] = out["dX3"]
    return out


def model_heads(c, fault=None):
    o = model_chain_generic(c["M"], c["dz"], [c["dd"], c["hD"]], [c["wrgb"], c["wext"]], [c["g_rgb0"], c["Tm0"]],
                            [c["g_brgb0"], c["svec0"]], fault)
    return dict(g_rgb=o["gW0"], g_brgb=o["gb0"], Tm=o["gW1"], svec=o["gb1"], dh=o["dX1"], dzd=o["dX0"])


def model_pe_ends(c, fault=None):
    M, nf = c["M"], c["n_freq"]
    tiles = (M + 127) // 128
    nwg = min(tiles, 512)
    dha, dhb, pe, wa, wb = (bf16_val(c[k], np.float32) for k in ("dha", "dhb", "pe", "wa", "wb"))
    pa, pb_, pg = np.zeros((nwg, 64, 63), np.float32), np.zeros((nwg, 64, 63), np.float32), np.zeros((nwg, 64), np.float32)
    d_xyz = np.full((M, 3), np.nan, np.float32)
    for g in range(nwg):
        for t in range(g, tiles, nwg):
            r0 = t * 128
            nv = min(128, M - r0)
            if fault == "short_row" and nv < 128:
                nv -= 1
            if nv <= 0:
                continue
            a, b, p = dha[r0:r0 + nv], dhb[r0:r0 + nv], pe[r0:r0 + nv, :63]
            pa[g] += a.T @ p
            pb_[g] += b.T @ p
            for rg in range(2 if fault == "db_half" else 4):
                pg[g] += b[32 * rg:32 * rg + 32].sum(0, dtype=np.float32)
            dpe = a @ wa + b @ wb
            x = c["xyz"][r0:r0 + nv]
            d = dpe[:, :3].copy()
            for k in range(nf):
                f = np.float32(2.0 ** k)
                d += (c["win"][k] * f) * (np.cos(f * x) * dpe[:, 3 + 6 * k:6 + 6 * k] - np.sin(f * x) * dpe[:, 6 + 6 * k:9 + 6 * k])
            d_xyz[r0:r0 + nv] = d
    return dict(gWa=c["gWa0"] + reduce_partials(pa, fault), gWb=c["gWb0"] + reduce_partials(pb_, fault),
                gb_b=c["gbb0"] + reduce_partials(pg, fault), d_xyz=d_xyz)


def model_signmap(bbits, ld_bits, fault=None):
    """The dW form's by-product: k-tiles of 64 rows of B; bytes outside rows < K, columns < N keep 0xAA."""
    K, N = bbits.shape
    out = np.full((K, ld_bits), 0xAA, np.uint8)
    for k0 in range(0, K, 64):
        rows = np.arange(k0, min(k0 + 64, K))
        src = rows
        if fault == "bits_wrong_rows" and len(rows) < 64:
            src = np.where(rows + 1 < K, rows + 1, rows - 1)
        tile = np.where((src >= 0)[:, None], bbits[np.maximum(src, 0)], 0).astype(np.uint16)
        out[rows, :N // 8] = np.packbits(keep_mask(tile), axis=1, bitorder="little")
    return out


def expected_bits(truth, stored_bf16):
    """The bit patterns an exact-kind output must have."""
    return bf16_bits(truth) if stored_bf16 else f32_bits(np.asarray(truth, np.float64).astype(np.float32))


BF16_OUT = frozenset(("dX", "dh", "dzd", "dX0", "dX1", "dX2", "dX3"))


def compare(ref, got, label="", show=True):
    """Every output of `got` against `ref`: name -> (figure, ok).  Bound None: the bit patterns are equal, figure = the number of
    elements that differ.  Else figure = the worst |got - truth| / bound (fraction_f32; fraction_bf16 for a bf16 output) and
    ok = every element inside its bound, with equal bit patterns where the bound is 0.  Prints one line (pytest -s)."""
    res = {}
    for name, g in got.items():
        truth, bound = ref[name]
        if bound is None:
            want = expected_bits(truth, name in BF16_OUT)
            have = np.ascontiguousarray(g, np.uint16) if name in BF16_OUT else f32_bits(g)
            bad = int((have != want).sum())
            res[name] = (bad, bad == 0)
        elif name in BF16_OUT:
            res[name] = fraction_bf16(g, truth, bound)
        else:
            frac, ok = fraction_f32(g, truth, bound)
            zero = bound == 0                                   # exact statements: the bit patterns
            res[name] = (frac, ok and bool((f32_bits(g)[zero] == expected_bits(truth, False)[zero]).all()))
    if show:
        print(f"  {label}: " + ", ".join(f"{k} {'=' if ref[k][1] is None else ''}{v[0]:.3g}{'' if v[1] else ' FAIL'}"
                                         for k, v in res.items()))
    return res
