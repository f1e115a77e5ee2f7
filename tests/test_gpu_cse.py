"""GPU checks of the DensePose-CSE matching (moda_amd/cse.py, csrc/cse_kernels.hip) against the float64 oracle tests/cse_numpy.py
within the bounds it states, and against the reference's float64 records (tests/golden/g34_cse.npz).

Arg-max acceptance: for EVERY query the returned index j must satisfy score64(j) >= max64 - bound (bound: cse_numpy's per-query
2 gamma_16 max_j sum |q_k c_jk|); where a margin was proven by the generator, or the scores are exact small integers, the index
must equal the oracle's."""
import numpy as np
import pytest
import torch

import cse_numpy as O
from moda_amd import cse
from test_cse_oracle import FLOW, G, OOD, RS, live_rows, rs_inputs

pytestmark = pytest.mark.gpu
QT, CT = cse.QUERY_TILE, cse.CAND_TILE
M_SEAM = 3 * CT + 40                                                       # forced to 2 ranges: [0, 2 CT) and [2 CT, M)
RANGE = 2 * CT


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def assert_accepted(q, c, idx, chunk=1024):
    """q (N,16), c (M,16), idx (N,): the acceptance rule, in row chunks so that the float64 scores stay small."""
    idx = np.asarray(idx)
    assert idx.shape == (q.shape[0],) and (idx >= 0).all() and (idx < c.shape[0]).all()
    for i in range(0, q.shape[0], chunk):
        s = O.scores64(q[i:i + chunk], c)
        ok = O.accepted(s, O.argmax_bound(q[i:i + chunk], c), idx[i:i + chunk])
        assert ok.all(), (i + int(np.argmin(ok)), "score below max64 - bound")


def test_plan_of_the_seam_cases():
    assert cse.argmax_splits(1, 40, M_SEAM, 2) == (2, RANGE)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("form", ["ood", "flow"])
def test_argmax_shape_grid(form, B):
    rng = np.random.default_rng(B * 7 + len(form))
    for N in (1, 31, 32, 33, 64, 65, QT, QT + 1):
        for M in (1, 63, 64, 65, CT, CT + 1, 12544):
            c = rng.standard_normal((B, 16, M)).astype(np.float32)         # the (16, h w) image layout
            if form == "ood":                                              # one (N,16) table against every frame
                q = rng.standard_normal((N, 16)).astype(np.float32)
                idx = host(cse.feat_argmax(dev(q), dev(c).transpose(1, 2)))
                qs = [q] * B
            else:                                                          # per-batch queries, image layout as well
                q = rng.standard_normal((B, 16, N)).astype(np.float32)
                idx = host(cse.feat_argmax(dev(q).transpose(1, 2), dev(c).transpose(1, 2)))
                qs = [q[b].T for b in range(B)]
            assert idx.shape == (B, N)
            for b in range(B):
                assert_accepted(qs[b], c[b].T, idx[b])


def test_argmax_row_major_candidates_and_unbatched():
    rng = np.random.default_rng(5)
    q, c = rng.standard_normal((70, 16)).astype(np.float32), rng.standard_normal((CT + 9, 16)).astype(np.float32)
    idx = host(cse.feat_argmax(dev(q), dev(c)))
    assert idx.shape == (70,)
    assert_accepted(q, c, idx)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("pos", [0, M_SEAM - 1, CT - 1, CT, RANGE - 1, RANGE])
def test_argmax_placed_winner(pos, splits):
    rng = np.random.default_rng(pos)
    q = np.abs(rng.standard_normal((QT + 5, 16))).astype(np.float32) + 0.1
    c = rng.uniform(-1, 1, (M_SEAM, 16)).astype(np.float32)
    c[pos] = 5.0
    idx = host(cse.feat_argmax(dev(q), dev(c), splits=splits))
    assert (idx == pos).all()


def int_case(rng, N=QT + 3, M=M_SEAM):
    """Small integers: every score is exact in fp32 and in float64."""
    q = rng.integers(1, 4, (N, 16)).astype(np.float32)
    c = rng.integers(-2, 3, (M, 16)).astype(np.float32)
    return q, c


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("pair", [(5, 9), (CT - 1, CT), (RANGE - 1, RANGE), (3, RANGE + 7), (M_SEAM - 2, M_SEAM - 1)])
def test_argmax_duplicate_candidates_give_the_lowest_index(pair, splits):
    q, c = int_case(np.random.default_rng(pair[0]))
    c[pair[0]] = c[pair[1]] = 3.0
    idx = host(cse.feat_argmax(dev(q), dev(c), splits=splits))
    assert (idx == pair[0]).all()
    assert np.array_equal(idx, O.argmax_rule(O.scores64(q, c)))


@pytest.mark.parametrize("splits", [1, 2])
def test_argmax_exact_ties_follow_the_oracle(splits):
    """Random small integers: many exact ties at every position, all resolved to the lowest index."""
    rng = np.random.default_rng(11)
    q = rng.integers(-1, 2, (QT + 3, 16)).astype(np.float32)
    c = rng.integers(-1, 2, (M_SEAM, 16)).astype(np.float32)
    s = O.scores64(q, c)
    assert ((s == s.max(1, keepdims=True)).sum(1) > 1).any()
    assert np.array_equal(host(cse.feat_argmax(dev(q), dev(c), splits=splits)), O.argmax_rule(s))


@pytest.mark.parametrize("splits", [1, 2])
def test_argmax_zero_rows_negative_remainder_signed_zero(splits):
    q, c = int_case(np.random.default_rng(3))
    c = -np.abs(c) - 1
    c[[7, 300, RANGE + 1]] = 0.0                                           # the first zero row wins over the negative rest
    assert (host(cse.feat_argmax(dev(q), dev(c), splits=splits)) == 7).all()
    c[7], c[300], c[4] = 0.0, -0.0, -0.0                                   # -0 counts as +0: now row 4
    assert (host(cse.feat_argmax(dev(q), dev(c), splits=splits)) == 4).all()
    qz = q.copy()
    qz[:, ::2] = -0.0
    qz[:, 1::2] = 0.0                                                      # every score is a zero of some sign: index 0
    assert (host(cse.feat_argmax(dev(qz), dev(c), splits=splits)) == 0).all()


@pytest.mark.parametrize("splits", [1, 2])
def test_argmax_nan_beats_numbers_lowest_nan_wins(splits):
    q, c = int_case(np.random.default_rng(4))
    c[10] = 3.0                                                            # the best number
    c[RANGE + 3, 2] = np.nan
    assert (host(cse.feat_argmax(dev(q), dev(c), splits=splits)) == RANGE + 3).all()
    c[70, 15] = np.nan
    assert (host(cse.feat_argmax(dev(q), dev(c), splits=splits)) == 70).all()
    c[70 + 32, 0] = np.nan                                                 # the same lane of the next column block
    assert (host(cse.feat_argmax(dev(q), dev(c), splits=splits)) == 70).all()
    assert np.array_equal(O.argmax_rule(O.scores64(q, c)), np.full(q.shape[0], 70))


def test_argmax_split_unsplit_and_reruns_identical():
    rng = np.random.default_rng(12)
    q = dev(rng.standard_normal((300, 16)).astype(np.float32))
    c = dev(rng.standard_normal((2, 16, 12544)).astype(np.float32)).transpose(1, 2)
    c[0, 5000:5100] = c[0, 100:200]                                        # exact duplicates far apart
    assert cse.argmax_splits(2, 300, 12544)[0] > 1
    base = cse.feat_argmax(q, c, splits=1)
    for splits in (0, 0, 2, 7, 49):
        assert torch.equal(cse.feat_argmax(q, c, splits=splits), base), splits
    assert torch.equal(cse.feat_argmax(q, c, splits=1), base)


# ---- resample -------------------------------------------------------------------------------------------------------------
def check_resample(feats, bbox, kaug, target, normalize=False, rows=None):
    got = host(cse.resample_dp(dev(feats), dev(bbox), dev(kaug), target, normalize=normalize))
    want, bound = O.resample_dp(feats, bbox, kaug, target, normalize=normalize)
    rows = list(range(feats.shape[0])) if rows is None else rows
    assert got.shape == want.shape and np.isfinite(got).all()
    excess = np.abs(got[rows] - want[rows]) - bound[rows]
    assert excess.max() <= 0, float(excess.max())
    return got


@pytest.mark.parametrize("name", RS)
def test_resample_stored_cases(name):
    feats, bbox, kaug, target = rs_inputs(name)
    rows = live_rows(name)
    got = check_resample(feats, bbox, kaug, target, rows=rows)
    assert np.abs(got[rows] - G[f"rs/{name}/out64"][rows]).max() <= O.resample_dp(feats, bbox, kaug, target)[1][rows].max() + 1e-10
    if name == "grid":
        check_resample(feats, bbox, kaug, target, normalize=True)
    if name == "mixed":                                                    # the grid branch for all rows; the degenerate row is zeros
        assert (got[0] == 0).all() and np.abs(got[1]).max() > 0
    if name == "outside":                                                  # zero padding where the crop leaves the source
        assert (got == 0).any() and (G[f"rs/{name}/out64"][got == 0] == 0).all()


@pytest.mark.parametrize("hs,ws,target,bs", [(112, 112, 512, 1), (112, 112, 64, 2), (5, 5, 7, 3), (3, 1, 4, 2), (3, 2, 5, 2)])
@pytest.mark.parametrize("branch", ["interp", "grid"])
def test_resample_seeded_grid(branch, hs, ws, target, bs):
    rng = np.random.default_rng(hs * 31 + ws + target)
    feats = rng.standard_normal((bs, 16, hs, ws)).astype(np.float32)
    kaug = (np.abs(rng.standard_normal((bs, 4))) + np.asarray([1.0, 1.0, 5.0, 5.0])).astype(np.float32)
    bbox = np.zeros((bs, 4), np.float32)
    if branch == "grid":
        lo = rng.uniform(-20, 60, (bs, 2))
        bbox = np.concatenate([lo, lo + rng.uniform(40, 200, (bs, 2))], 1).astype(np.float32)
    check_resample(feats, bbox, kaug, target)


def test_resample_normalize_with_zero_pixels():
    rng = np.random.default_rng(8)
    feats = rng.standard_normal((2, 16, 12, 12)).astype(np.float32)
    feats[:, :, :5] = 0
    kaug = np.asarray([[1.0, 1.0, 0.0, 0.0]] * 2, np.float32)
    for bbox in (np.zeros((2, 4), np.float32), np.asarray([[0, 0, 112, 112]] * 2, np.float32)):
        got = check_resample(feats, bbox, kaug, 12, normalize=True)
        assert (got[:, :, :3] == 0).all()                                  # 0 / max(0, 1e-12), not NaN
        n = np.linalg.norm(got[:, :, 8:], axis=1)
        assert np.abs(n - 1).max() < 1e-5


def test_resample_graph_replay_follows_new_contents():
    rng = np.random.default_rng(9)
    feats = rng.standard_normal((2, 16, 24, 24)).astype(np.float32)
    boxes = [np.zeros((2, 4), np.float32), np.asarray([[42, 63, 137, 150], [8, 26, 131, 144]], np.float32),
             np.asarray([[0, 0, 0, 0], [12, 27, 94, 105]], np.float32), np.zeros((2, 4), np.float32)]
    kaugs = [np.asarray([[1.7, 1.6, 40, 60], [2.2, 2.1, 10, 25]], np.float32), np.asarray([[1.2, 1.3, 20, 30], [2.0, 1.9, 15, 5]], np.float32)]
    f, b, k = dev(feats), dev(boxes[0]), dev(kaugs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cse.resample_dp(f, b, k, 16, normalize=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cse.resample_dp(f, b, k, 16, normalize=True)
    for i, box in enumerate(boxes):                                        # across the branch, both ways
        ka = kaugs[i % 2]
        b.copy_(dev(box))
        k.copy_(dev(ka))
        graph.replay()
        want, bound = O.resample_dp(feats, box, ka, 16, normalize=True)
        rows = [r for r in range(2) if np.abs(box).sum() == 0 or np.abs(box[r]).sum() != 0]
        assert (np.abs(host(out)[rows] - want[rows]) <= bound[rows]).all(), i
        assert (want[rows] != 0).mean() > 0.05                             # the crop samples the source, not only padding


# ---- ood_check_cse --------------------------------------------------------------------------------------------------------
def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


@pytest.mark.parametrize("name", OOD)
def test_ood_stored_cases(name):
    feats, embed, dp_idx = G[f"ood/{name}/feats"], G[f"ood/{name}/embed"], G[f"ood/{name}/dp_idx"]
    valid, err, status = cse.ood_check_cse(dev(feats), dev(embed), dev(dp_idx), return_status=True)
    assert valid.dtype == torch.bool and err.dtype == torch.float32 and valid.is_cuda and err.is_cuda
    _, _, bound, _ = O.ood_check_cse(feats, embed, dp_idx)
    want = G[f"ood/{name}/err64"]
    err = host(err).astype(np.float64)
    assert same_nan(err, want) and np.isnan(err[2]) and not host(valid)[2]  # the empty mask
    assert np.nanmax(np.abs(err - want) - bound) <= 0
    assert np.array_equal(host(valid), G[f"ood/{name}/valid64"])
    assert int(status.item()) == 0
    for dt in (torch.int32, torch.float32):                                # the reference takes any integer-valued dp_idx
        v2, e2 = cse.ood_check_cse(dev(feats), dev(embed), dev(dp_idx).to(dt))
        assert torch.equal(v2.cpu(), torch.from_numpy(host(valid))) and same_nan(host(e2), err) and np.array_equal(host(e2)[:2], err[:2].astype(np.float32))


def test_ood_bad_indices_are_counted_not_read():
    feats, embed = G["ood/w16/feats"], G["ood/w16/embed"]
    dp_idx = G["ood/w16/dp_idx"].copy()                                    # 16 -> 16: every value is sampled exactly once
    N = embed.shape[0]
    dp_idx[0, 2, 3], dp_idx[0, 9, 9], dp_idx[1, 0, 0], dp_idx[1, 15, 15] = N, -1, 2 ** 31 - 1, -2 ** 31
    valid, err, status = cse.ood_check_cse(dev(feats), dev(embed), dev(dp_idx), return_status=True)
    assert int(status.item()) == 4
    wv, we, bound, bad = O.ood_error_from_idx(G["ood/w16/idx64"], dp_idx, 16, 16)
    assert bad == 4 and np.nanmax(np.abs(host(err) - we) - bound) <= 0 and np.array_equal(host(valid), wv)


def test_ood_seeded_112_both_sides_of_the_threshold():
    rng = np.random.default_rng(112)
    h, N, bs = 112, 5004, 2
    feats = rng.standard_normal((bs, 16, h, h))
    feats = (feats / np.linalg.norm(feats, axis=1, keepdims=True)).astype(np.float32)
    feats[:, :, :20] = 0                                                   # outside the box: zero rows that tie at 0
    embed = rng.standard_normal((N, 16))
    embed = (embed / np.linalg.norm(embed, axis=1, keepdims=True)).astype(np.float32)
    f = dev(feats)
    idx = host(cse.feat_argmax(dev(embed), f.view(bs, 16, h * h).transpose(1, 2)))
    for b in range(bs):
        assert_accepted(embed, feats[b].reshape(16, -1).T, idx[b])
    lab = np.zeros(h * h, np.int64)
    lab[idx[0][::-1]] = np.arange(N)[::-1]                                 # frame 0: every labelled pixel is its label's match
    dp_idx = rng.integers(1, N, (bs, 2 * h, 2 * h))
    dp_idx[0] = np.repeat(np.repeat(lab.reshape(h, h), 2, 0), 2, 1)        # 224 -> 112 by the nearest rule
    valid, err, status = cse.ood_check_cse(f, dev(embed), dev(dp_idx), return_status=True)
    wv, we, bound, bad = O.ood_error_from_idx(idx, dp_idx, h, h)
    assert bad == 0 and int(status.item()) == 0
    assert np.abs(host(err) - we).max() <= bound.max() and (np.abs(host(err) - we) <= bound).all()
    assert we[0] < 12 < we[1] and host(valid).tolist() == [True, False] == wv.tolist()


# ---- compute_flow_cse / match2flo -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FLOW)
def test_flow_stored_cases(name):
    a, b = G[f"flow/{name}/a"], G[f"flow/{name}/b"]
    wa, wb, size = G[f"flow/{name}/warp_a"], G[f"flow/{name}/warp_b"], int(G[f"flow/{name}/img_size"])
    ma = host(cse.feat_argmax(dev(a).flatten(1).t(), dev(b).flatten(1).t()))
    mb = host(cse.feat_argmax(dev(b).flatten(1).t(), dev(a).flatten(1).t()))
    assert np.array_equal(ma, G[f"flow/{name}/ma64"]) and np.array_equal(mb, G[f"flow/{name}/mb64"])   # margins proven by the generator
    fa, fb = cse.compute_flow_cse(dev(a), dev(b), dev(wa), dev(wb), size)
    _, ba, _, bb, _, _, _ = O.compute_flow_cse(a, b, wa, wb, size)
    assert (np.abs(host(fa) - G[f"flow/{name}/fa64"]) <= ba + 1e-10).all()
    assert (np.abs(host(fb) - G[f"flow/{name}/fb64"]) <= bb + 1e-10).all()
    w = a.shape[-1]
    f2 = cse.match2flo(dev(ma.astype(np.int64)), w, size, dev(wa), dev(wb), "cuda")
    assert torch.equal(f2, fa)


def test_flow_identical_frames_is_the_warp_difference():
    rng = np.random.default_rng(21)
    w, size = 20, 200
    a = rng.standard_normal((16, w, w))
    a = (a / np.linalg.norm(a, axis=0, keepdims=True)).astype(np.float32)
    wa = np.asarray([[3.0, 0, 40.0], [0, 2.5, 70.0], [0, 0, 1]], np.float32)
    wb = np.asarray([[2.5, 0, 60.0], [0, 3.5, 50.0], [0, 0, 1]], np.float32)
    m = host(cse.feat_argmax(dev(a).flatten(1).t(), dev(a).flatten(1).t()))
    assert np.array_equal(m, np.arange(w * w))
    fa, fb = cse.compute_flow_cse(dev(a), dev(a.copy()), dev(wa), dev(wb), size)
    wfa, ba = O.match2flo(np.arange(w * w), w, size, wa, wb)
    wfb, bb = O.match2flo(np.arange(w * w), w, size, wb, wa)
    assert (np.abs(host(fa) - wfa) <= ba).all() and (np.abs(host(fb) - wfb) <= bb).all()
    assert np.abs(wfa).max() > 0.01
