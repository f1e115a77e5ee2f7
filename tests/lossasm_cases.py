"""Inputs of the loss-stage tests, plain numpy: built once here so that the conditions tests/test_lossasm_oracle.py asserts on the
float64 restatement (exact sums, margins to the threshold, share of clamp-edge triples) hold for what tests/test_gpu_lossasm.py
runs on the device."""
import numpy as np

POSITIVE_COUNTS = (0, 1, 2, 3, 64, 65, 255, 256, 257, 1025)       # the median kernel's wave (64) and block (1024) seams


def dyadic(rng, shape, lo=1, hi=16 * 1024):
    """Multiples of 2^-10 below 2^4: sums of a few thousand of them are exact in fp32 and float64, in any order."""
    return (rng.integers(lo, hi, size=shape) / 1024.0).astype(np.float32)


def line_calls_small(seed=3):
    """num_frames=7, img_size=8, N=24: three calls; every errid repeated 2-4 times in shuffled order (last-wins decides); the
    second call stores 0 over a positive value and holds one out-of-range id; the third lifts one frame far above 10 medians."""
    rng = np.random.default_rng(seed)
    T, S, N = 7, 8, 24
    calls = []
    for c in range(3):
        ids = rng.choice(T * S, size=8, replace=False)
        if c == 1:
            ids[0] = calls[0][0][0]                                  # a slot the first call filled
        errid = np.concatenate([np.repeat(ids[:4], 2), np.repeat(ids[4:6], 4), np.repeat(ids[6:], 4)])
        vals = dyadic(rng, N)
        order = rng.permutation(N)
        errid, vals = errid[order], vals[order]
        frameid = errid // S
        if c == 1:
            vals[errid == ids[0]] = 0.0                              # a zero over a positive value
            errid[5] = T * S                                         # outside the table: skipped and counted
        if c == 2:
            vals[frameid == frameid[0]] *= 64
        calls.append((errid.astype(np.int64), frameid.astype(np.int64), vals))
    return T, S, calls


def line_case_counts(K, seed=5):
    """One call that leaves exactly K frames with a positive mean, two of them tied, one (K >= 3) above ten medians; every id is
    written twice with different values."""
    rng = np.random.default_rng(seed + K)
    T, S = max(K + 3, 7), 8
    frames = rng.permutation(T)[:K]
    slots = frames * S + rng.integers(0, S, size=K)
    last = dyadic(rng, K, lo=1024, hi=4096)
    if K >= 2:
        last[1] = last[0]                                            # tied means
    if K >= 3:
        last[2] = np.float32(1000.0)                                 # > 10 * any median of values below 4
    zero_frames = np.setdiff1d(np.arange(T), frames)[:2]
    errid = np.concatenate([slots, slots, zero_frames * S])
    vals = np.concatenate([dyadic(rng, K), last, np.zeros(len(zero_frames), np.float32)])    # the second write wins
    keep_order = np.concatenate([rng.permutation(K), K + rng.permutation(K + len(zero_frames))])
    errid, vals = errid[keep_order], vals[keep_order]
    return T, S, errid.astype(np.int32), (errid // S).astype(np.int32), vals.astype(np.float32)


def threshold_pair():
    """(v0, v_at, v_above): with one slot per frame, mean(v_at) == 10 * median exactly in float64 (strict >: not flagged) and
    v_above, one input step (2^-10) higher, is above it.  Frames: three at v0 (the median), one at v_at or v_above."""
    for q in range(1024, 4096):
        v0 = q / 1024.0
        d = 1e-9 + 1.0
        if (10 * v0) / d == (v0 / d) * 10 and (10 * v0 + 2.0 ** -10) / d > (v0 / d) * 10:
            return np.float32(v0), np.float32(10 * v0), np.float32(10 * v0 + 2.0 ** -10)
    raise AssertionError("no dyadic value puts a frame exactly at ten medians")


def threshold_case(above):
    v0, v_at, v_above = threshold_pair()
    T, S = 7, 8
    errid = np.array([0, 8, 16, 24], np.int64) + 3
    vals = np.array([v0, v0, v0, v_above if above else v_at], np.float32)
    return T, S, errid, errid // S, vals


def line_case_random(seed=11):
    """img_size=512, random fp32 values (sums no longer exact): 7 frames, 2048 rays, one frame scaled above the threshold."""
    rng = np.random.default_rng(seed)
    T, S, N = 7, 512, 2048
    errid = rng.integers(0, T * S, size=N)
    vals = rng.random(N).astype(np.float32)
    vals[errid // S == 4] *= 40
    return T, S, errid.astype(np.int64), (errid // S).astype(np.int64), vals


def frame_threshold_case(bs, above):
    """History of three frames at v0; row 0 is a single selected ray whose flo_err is exactly 10 * v0 (strict >: not flagged) or
    one input step above it; the other rows lie at v0."""
    v0, v_at, v_above = threshold_pair()
    T, n = 9, 4
    hist = np.zeros(T, np.float32)
    hist[[1, 4, 6]] = v0
    x = np.full((bs, n), v0, np.float32)
    x[0, 0] = v_above if above else v_at
    mask = np.ones((bs, n), bool)
    mask[0, 1:] = False
    x[0, 1:] = 3.0                                                   # masked out
    return T, hist, x, mask, (np.arange(bs) + 2).astype(np.int64)


def frame_case_random(bs, seed=19):
    """Random fp32 values and history (sums no longer exact); row 0 scaled far above ten medians."""
    rng = np.random.default_rng(seed + bs)
    T, n = 300, 2048
    hist = rng.random(T).astype(np.float32)
    hist[rng.permutation(T)[:40]] = 0
    x = rng.random((bs, n)).astype(np.float32)
    x[0] *= 40
    mask = rng.random((bs, n)) > 0.3
    return T, hist, x, mask, rng.permutation(T)[:bs].astype(np.int64)


def frame_calls(bs, seed=21):
    """Three consecutive calls on one history of 9 frames that starts empty; the second holds an errid outside the table; in the
    third, row 0 lies far above ten medians of what the first two left."""
    rng = np.random.default_rng(seed + bs)
    T, n = 9, 37
    calls = []
    for c in range(3):
        x = dyadic(rng, (bs, n), lo=1024, hi=2048)
        if c == 2:
            x[0] *= 64
        mask = rng.random((bs, n)) > 0.3
        mask[:, 0] = True
        errid = rng.permutation(T)[:bs].astype(np.int64)
        if c == 1:
            errid[-1] = T + 3
        calls.append((x, mask, errid))
    return T, calls


def frame_case(bs, K, seed=17):
    """History with K positive entries (two tied), bs rows of 37 rays, dyadic; row 0 lies far above ten medians."""
    rng = np.random.default_rng(seed + 31 * K + bs)
    T, n = max(K + 3, 9), 37
    hist = np.zeros(T, np.float32)
    where = rng.permutation(T)[:K]
    hist[where] = dyadic(rng, K, lo=1024, hi=4096)
    if K >= 2:
        hist[where[1]] = hist[where[0]]
    x = dyadic(rng, (bs, n), lo=1024, hi=2048)
    x[0] *= 64
    mask = rng.random((bs, n)) > 0.3
    mask[:, 0] = True
    errid = rng.permutation(T)[:bs].astype(np.int64)
    if bs > 1:
        errid[-1] = errid[0]                                         # a repeated id: the last row's value stays
    return T, hist, x, mask, errid


def root_case(kind, seed=23):
    """rtk (T, 4, 4) fp32 and data_offset.  'videos': videos of 2, 3, 5, 64, 65 and 70 frames, smooth random walks; 'same':
    identical poses (upper clamp, zero translation difference); 'flip': steps of 180 degrees about changing axes (lower clamp)."""
    rng = np.random.default_rng(seed)
    if kind == "videos":
        off = (0, 2, 5, 10, 74, 139, 209)
    else:
        off = (0, 6)
    T = off[-1]
    rtk = np.zeros((T, 4, 4), np.float32)
    rtk[:, 3, 3] = 1
    R = np.eye(3)
    for f in range(T):
        if kind == "videos":
            w = rng.normal(size=3) * 0.3
            th = np.linalg.norm(w)
            k = w / th
            Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            R = R @ (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx)
            rtk[f, :3, :3] = R
            rtk[f, :3, 3] = rng.normal(size=3)
        elif kind == "same":
            rtk[f, :3, :3] = np.eye(3)
            rtk[f, :3, 3] = (0.25, -1.5, 3.0)
        else:                                                        # R_f = diag(1, (-1)^f, (-1)^f): (R0 R1^T)(R1 R2^T)^T = I ...
            s = -1.0 if f % 2 else 1.0
            rtk[f, :3, :3] = np.diag([1.0, s, s])
            rtk[f, :3, 3] = (0.5 * f, 0.0, f * f * 0.125)
    if kind == "flip":                                               # ... so break the symmetry: frames 0, 1, 2 = I, Rx(pi), I -> A = Rx(pi),
        rtk[2, :3, :3] = np.diag([-1.0, -1.0, 1.0])                  # B = Rx(pi) Rz(pi) = Ry(pi): <A, B> = 1 - 1 - 1 = -1, cos = -1
    return rtk, off


def assembly_case(N=37, seed=29):
    """Every term of the table over N = 37 rays, and options that switch every branch on (projection warm-up window (0, 0.4))."""
    rng = np.random.default_rng(seed)
    f = lambda *sh: np.abs(rng.normal(size=sh)).astype(np.float32)
    rendered = dict(img_loss_samp=f(N, 3), sil_loss_samp=f(N, 1), frnd_loss_samp=f(N, 1), flo_loss_samp=f(N, 1), feat_err=f(N, 1),
                    corr_err=f(N, 1), proj_err=f(N, 1), s3im_loss=f(), frame_cyc_dis=f(N), elastic_loss=f(N, 4), dis_reg=f(N, 2),
                    dis_reg_forward=f(N, 2), vis_loss=f(), eikonal_loss=f(), unc_pred=f(N, 1),
                    sil_coarse=rng.random((N, 1)).astype(np.float32),
                    sil_at_samp=(rng.random((N, 1)) > 0.3).astype(np.float32), vis_at_samp=(rng.random((N, 1)) > 0.1).astype(np.float32),
                    sil_at_samp_flo=rng.random((N, 1)) > 0.5)
    opts = dict(s3im_loss=True, use_corr=True, freeze_proj=True, proj_start=0.0, proj_end=0.4, eikonal_wt=0.05, feat_wt=0.2,
                total_wt=1.7, bone_loc_reg=0.0, warmup_steps=0.1)
    return rendered, opts


# (N, wide, empty): N = 37 lies under one wave, 64 fills one, 577 = 512 + 64 + 1 is one full eight-row block of the lane loop, one
# more wave row and a tail of one; `wide` gives the bool-masked and the unmasked term three columns beside img's; `empty` leaves
# the bool mask without a selected row (a NaN term and a NaN total)
TOTAL_LOSS_BITS_CASES = ((37, False, False), (64, True, False), (577, False, False), (577, True, False), (37, True, True),
                         (577, False, True))
TOTAL_LOSS_BITS_INPUTS = ("img_loss_samp", "sil_loss_samp", "frnd_loss_samp", "flo_loss_samp", "feat_err", "proj_err", "vis_loss",
                          "frame_cyc_dis")


def total_loss_bits_case(N, wide, empty):
    """`rendered` for total_loss with all eight terms: k = 1 and 3, no mask / float `> 0` / bool masks, the 0-dim vis_loss and the
    zero-weight feat term (feat_wt's default).  Plain normals, so every sum depends on the order it is formed in."""
    rng = np.random.default_rng(3100 + 7 * N + 2 * wide + empty)
    f = lambda *sh: np.abs(rng.normal(size=sh)).astype(np.float32)
    k = 3 if wide else 1
    return dict(img_loss_samp=f(N, 3), sil_loss_samp=f(N, 1), frnd_loss_samp=f(N, 1), flo_loss_samp=f(N, k), feat_err=f(N, 1),
                proj_err=f(N, 1), vis_loss=f(), frame_cyc_dis=f(N, k) if wide else f(N),
                sil_at_samp=(rng.random((N, 1)) > 0.3).astype(np.float32), vis_at_samp=(rng.random((N, 1)) > 0.1).astype(np.float32),
                sil_at_samp_flo=np.zeros((N, 1), bool) if empty else rng.random((N, 1)) > 0.5)
