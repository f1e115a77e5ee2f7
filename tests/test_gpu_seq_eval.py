"""GPU (-m gpu): the whole-sequence route of moda_amd/mesh_eval.py -- ragged / masked point-set launches, moda_icp_solve,
moda_icp_advance, moda_seq_metrics, iterative_closest_point_device and eval_sequence -- against the host route of the same
module and the float64 oracles tests/icpdev_numpy.py / tests/pointset_numpy.py.  u = 2^-24.

  ragged nn   the bars of check_nearest (5 u, 10 u, at most 0.1 % of the queries left out of the exact index comparison; the
              clouds are confirmed inside that cap on the CPU, tests/test_icpdev_oracle.py).  The padding rows are copies of
              a query, so reading one would win with distance 0.
  solve       against mesh_eval._align on the same sums: the output row is rounded once to fp32 (u / 2 relative per entry)
              and the two float64 SVDs differ by parts in 1e15, so 4 u max(1, |T|) where the alignment is well conditioned;
              where the covariance is rank deficient R is not unique: orthonormal with det +1 to 1e-6, and the same fit to
              1e-5 of the cloud size (the ICP bar of tests/test_gpu_mesh_eval.py).
  icp         iteration counts, flags and correspondences equal to the host route; R, T to 1e-5, rmse to 1e-5 bbox.
  sequence    per frame the bars of test_eval_mesh_matches_oracle."""
import functools

import numpy as np
import pytest
import torch

import icpdev_numpy as icn
import pointset_numpy as psn
from test_icpdev_oracle import RAGGED_LENS, ragged_case, stopping_batch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import moda_amd
    from moda_amd import mesh as M, mesh_eval as ME, _lib
    from gpu_helpers import T, DEV
    from test_gpu_mesh_eval import check_nearest, raw_nn, _sphere

U = 2.0 ** -24


def I32(a):
    return torch.as_tensor(np.asarray(a, np.int32)).to(DEV)


def raw_nn_ragged(x, y, lens, active, with_keys, d=None, i=None):
    B, N, Mm = x.shape[0], x.shape[1], y.shape[1]
    d = torch.empty((B, N), dtype=torch.float32, device=DEV) if d is None else d
    i = torch.empty((B, N), dtype=torch.int32, device=DEV) if i is None else i
    keys = torch.empty((B, N), dtype=torch.int64, device=DEV) if with_keys else None
    _lib.call("moda_nn_fwd_ragged", _lib.ptr(x), _lib.ptr(y), B, N, Mm, _lib.ptr(lens), _lib.ptr(active), _lib.ptr(d), _lib.ptr(i),
              _lib.ptr(keys), _lib.stream())
    return d, i


@pytest.mark.parametrize("N", [1, 1025])
def test_ragged_nearest(N):
    x, y = ragged_case(N)
    xt, yt, lens = T(x), T(y), I32(RAGGED_LENS)
    assert ME.nn_plan(3, N, 1025)[0] > 1                                     # the split route, and the unsplit one below
    d, i = raw_nn_ragged(xt, yt, lens, None, True)
    for b, n in enumerate(RAGGED_LENS):
        assert int(i[b].max()) < n and int(i[b].min()) >= 0                  # the padding was never a candidate
        check_nearest(x[b], y[b][:n], d[b], i[b])
    d1, i1 = raw_nn_ragged(xt, yt, lens, None, False)
    assert torch.equal(d1, d) and torch.equal(i1, i)
    # full lengths, all active: the bits of moda_nn_fwd
    full, ones = I32([1025] * 3), I32([1, 1, 1])
    for with_keys in (True, False):
        want = raw_nn(xt, yt, with_keys)
        for active in (None, ones):
            got = raw_nn_ragged(xt, yt, full, active, with_keys)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a skipped cloud keeps the bits it had
    for with_keys in (True, False):
        d0 = torch.full((3, N), 7.0, device=DEV)
        i0 = torch.full((3, N), -5, dtype=torch.int32, device=DEV)
        raw_nn_ragged(xt, yt, lens, I32([1, 0, 1]), with_keys, d0, i0)
        assert (d0[1] == 7.0).all() and (i0[1] == -5).all()
        assert torch.equal(d0[0], d[0]) and torch.equal(i0[2], i[2]) and torch.equal(d0[2], d[2])


def test_masked_moments_and_apply():
    x, y, _, _, _ = psn.icp_case(0, 5.0)
    xb, yb = T(np.stack([x] * 3)), T(np.stack([y] * 3))
    lens, active = I32([3000, 2000, 3000]), I32([1, 1, 0])
    _, idx = ME.nearest(xb, yb)
    sums = torch.full((3, 17), -3.0, dtype=torch.float64, device=DEV)
    partials = torch.empty((3, 256, 17), dtype=torch.float64, device=DEV)
    _lib.call("moda_icp_moments_ragged", _lib.ptr(xb), _lib.ptr(yb), _lib.ptr(idx), _lib.ptr(xb), 3, 1500, 3000, _lib.ptr(lens),
              _lib.ptr(active), _lib.ptr(partials), _lib.ptr(sums), _lib.stream())
    want = ME.icp_moments(xb, yb, idx, xb)
    assert torch.equal(sums[0], want[0]) and (sums[2] == -3.0).all()
    keep = (idx[1] < 2000).cpu().numpy()                                      # an index into the padding is skipped
    assert not keep.all()
    w1 = icn.moments(x[keep], y[idx[1].cpu().numpy()[keep]], x[keep])
    assert np.abs(sums[1].cpu().numpy() - w1).max() <= 1e-9
    rts = T(np.tile(np.array([[0, 1, 0, -1, 0, 0, 0, 0, 1, .1, .2, .3, 1.5]], np.float32), (3, 1)))
    out = torch.full_like(xb, 9.0)
    _lib.call("moda_sim3_apply_masked", _lib.ptr(xb), _lib.ptr(rts), 3, 1500, _lib.ptr(active), _lib.ptr(out), _lib.stream())
    ref = torch.empty_like(xb)
    _lib.call("moda_sim3_apply", _lib.ptr(xb), _lib.ptr(rts), 3, 1500, _lib.ptr(ref), _lib.stream())
    assert torch.equal(out[:2], ref[:2]) and (out[2] == 9.0).all()


def _solve_cases():
    """-> (name, X, Yn, estimate_scale, allow_reflection, well_conditioned)"""
    cases = []
    for seed, deg in ((0, 5.0), (1, 10.0), (2, 15.0), (3, 10.0)):
        X, Y, subset, _, _ = psn.icp_case(seed, deg)
        cases.append((f"icp_case{seed}", X, Y[subset], False, False, True))
        cases.append((f"icp_case{seed}_first", X, Y[psn.nearest(X, Y)[1]], False, False, True))
    X, Y, subset, _, _ = psn.icp_case(3, 5.0, scale=1.1)
    cases.append(("scale1.1", X, Y[subset], True, False, True))
    X, Y, subset, _, _ = psn.icp_case(4, 10.0)
    mirrored = (Y[subset] * np.array([1, 1, -1], np.float32)).astype(np.float32)
    cases.append(("mirrored", X, mirrored, False, False, True))
    cases.append(("mirrored_reflection_allowed", X, mirrored, False, True, True))
    rng = np.random.default_rng(7)
    Rt, Tt = psn.rotation((3, 1, 2), 20.0), np.array([0.05, -0.02, 0.03])
    P = np.concatenate([rng.uniform(-0.3, 0.3, (500, 2)), np.zeros((500, 1))], 1).astype(np.float32)
    cases.append(("planar", P, (P @ Rt + Tt).astype(np.float32), False, False, False))
    Lc = (rng.uniform(-0.3, 0.3, (500, 1)) * np.array([[1.0, 2.0, -0.5]])).astype(np.float32)
    cases.append(("collinear", Lc, (Lc @ Rt + Tt).astype(np.float32), False, False, False))
    One = np.tile(np.array([[0.1, -0.2, 0.3]], np.float32), (500, 1))
    cases.append(("x_is_its_mean", One, rng.uniform(-0.3, 0.3, (500, 3)).astype(np.float32), False, False, False))
    cases.append(("all_zero", np.zeros((500, 3), np.float32), np.zeros((500, 3), np.float32), False, False, False))
    return cases


def test_icp_solve_matches_align():
    cases = _solve_cases()
    sums = np.stack([icn.moments(X, Yn) for _, X, Yn, *_ in cases])
    st = torch.as_tensor(sums).to(DEV)
    # every case is solved alone (its own flags and its own n), over a range of sweep counts; 0 = the library's count
    worst = {}
    for sweeps in (1, 2, 3, 4, 5, 6, 7, 8, 0):
        for k, (name, X, Yn, est, refl, well) in enumerate(cases):
            rts = ME._icp_solve(st[k:k + 1], len(X), est, refl, sweeps=sweeps)[0].cpu().numpy().astype(np.float64)
            R, Tv, s = rts[:9].reshape(3, 3), rts[9:12], rts[12]
            Ra, Ta, sa = ME._align(sums[k], len(X), est, refl)
            if well:
                err = max(np.abs(R - Ra).max(), np.abs(Tv - Ta).max(), abs(s - sa)) / max(1.0, np.abs(Ta).max())
                worst[sweeps] = max(worst.get(sweeps, 0.0), err)
                if sweeps == 0:
                    assert err <= 4 * U, (name, err / U)
                    assert abs(np.linalg.det(R) - (-1.0 if name == "mirrored_reflection_allowed" else 1.0)) <= 1e-6
            elif sweeps == 0:
                size = max(float(np.abs(X).max()), float(np.abs(Yn).max()), 1e-30)
                Xd = X.astype(np.float64)
                fit = np.abs((s * Xd @ R + Tv) - (sa * Xd @ Ra + Ta)).max()
                print(name, "max |R^T R - I|", np.abs(R.T @ R - np.eye(3)).max(), "det", np.linalg.det(R), "fit difference / size",
                      fit / size)
                assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R) - 1.0) <= 1e-6
                assert fit <= 1e-5 * size and s == 1.0
    for sweeps, e in worst.items():
        print("sweeps", sweeps or "default", "max error of the well-conditioned cases in u:", e / U)
    # the active mask: a skipped cloud's row keeps its bits
    rts = torch.full((len(cases), 13), 5.0, device=DEV)
    act = I32([k % 2 for k in range(len(cases))])
    ME._icp_solve(st, 1500, active=act, out=rts)
    assert (rts[0::2] == 5.0).all() and not (rts[1::2] == 5.0).any()


@functools.lru_cache(maxsize=None)
def _host_icp(seed, degrees):
    X, Y, subset, R, T_ = psn.icp_case(seed, degrees)
    sol = moda_amd.iterative_closest_point(T(X)[None], T(Y)[None])
    return X, Y, subset, sol


@pytest.mark.parametrize("seed,degrees", [(0, 5.0), (1, 10.0), (2, 15.0), (3, 10.0)])
def test_device_icp_equals_host_icp(seed, degrees):
    X, Y, subset, host = _host_icp(seed, degrees)
    sol = moda_amd.iterative_closest_point_device(T(X)[None], T(Y)[None])
    bbox = float((Y.max(0) - Y.min(0)).max())
    print(seed, "iterations", int(sol.iterations[0]), len(host.t_history), "rmse", float(sol.rmse[0]), float(host.rmse[0]),
          "max |dR|", float((sol.RTs.R - host.RTs.R).abs().max()), "max |dT|", float((sol.RTs.T - host.RTs.T).abs().max()))
    assert isinstance(sol, moda_amd.ICPSolution) and sol.t_history is None
    assert sol.converged.dtype == torch.bool and sol.converged.shape == (1,) and sol.iterations.shape == (1,)
    assert int(sol.iterations[0]) == len(host.t_history) and bool(sol.converged[0]) is host.converged is True
    assert torch.equal(ME.nearest(sol.Xt[0], T(Y))[1], ME.nearest(host.Xt[0], T(Y))[1])
    assert np.array_equal(sol.idx[0].cpu().numpy(), subset)
    assert float((sol.RTs.R - host.RTs.R).abs().max()) <= 1e-5 and float((sol.RTs.T - host.RTs.T).abs().max()) <= 1e-5
    assert abs(float(sol.rmse[0]) - float(host.rmse[0])) <= 1e-5 * bbox and float(sol.RTs.s[0]) == 1.0
    if seed == 0:
        one = moda_amd.iterative_closest_point_device(T(X)[None], T(Y)[None], max_iterations=1, keep_history=True)
        assert not bool(one.converged[0]) and int(one.iterations[0]) == 1 and len(one.t_history) == 1
        again = moda_amd.iterative_closest_point_device(T(X)[None], T(Y)[None], init_transform=sol.RTs)
        assert bool(again.converged[0]) and int(again.iterations[0]) <= 2
        assert torch.allclose(again.RTs.R, sol.RTs.R, atol=1e-6)


def test_history_holds_every_iteration():
    """keep_history: entry k is the transform after iteration k + 1, i.e. what a run stopped there returns -- in a batch under
    the per-element rule too, where a cloud that has stopped keeps repeating its last transform."""
    X, Y = stopping_batch()
    xt, yt = T(X), T(Y)
    full = moda_amd.iterative_closest_point_device(xt, yt, per_element=True, keep_history=True)
    n = int(full.iterations.max())
    assert len(full.t_history) == 100 and n >= 5                              # check_every = 0: all rounds are issued
    for k in (0, 1, 2, n - 1):
        cut = moda_amd.iterative_closest_point_device(xt, yt, per_element=True, max_iterations=k + 1)
        for got, want in zip(full.t_history[k], cut.RTs):
            assert torch.equal(got, want), k
    for got, want in zip(full.t_history[-1], full.RTs):
        assert torch.equal(got, want)
    assert not torch.equal(full.t_history[0].R[1], full.t_history[n - 1].R[1])   # the entries are not views of one buffer
    assert not torch.equal(full.t_history[0].T[1], full.t_history[n - 1].T[1])
    early = moda_amd.iterative_closest_point_device(xt, yt, per_element=True, keep_history=True, check_every=1)
    assert len(early.t_history) == n and all(torch.equal(a, b) for a, b in zip(early.t_history[-1], full.RTs))


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(torch.equal(p[rows_a], q[rows_b]) for p, q in
               ((a.Xt, b.Xt), (a.RTs.R, b.RTs.R), (a.RTs.T, b.RTs.T), (a.RTs.s, b.RTs.s), (a.rmse, b.rmse),
                (a.iterations, b.iterations), (a.converged, b.converged)))


def test_stopping_rules():
    X, Y = stopping_batch()
    xt, yt = T(X), T(Y)
    per = moda_amd.iterative_closest_point_device(xt, yt, per_element=True)
    print("per element: iterations", per.iterations.tolist(), "rmse", per.rmse.tolist())
    for b in range(3):                                                        # exactly its own batch of one
        single = moda_amd.iterative_closest_point_device(xt[b:b + 1], yt[b:b + 1], per_element=True)
        assert _same(per, single, slice(b, b + 1))
    assert per.converged.all() and float(per.rmse[0]) == 0.0 and int(per.iterations[0]) == 2   # X == Y: `relative` is 1 at first
    assert len(set(per.iterations.tolist())) > 1
    host = moda_amd.iterative_closest_point(xt, yt)
    both = moda_amd.iterative_closest_point_device(xt, yt, per_element=False)
    print("all elements: iterations", both.iterations.tolist(), "host", len(host.t_history))
    assert both.iterations.tolist() == [len(host.t_history)] * 3 and both.converged.all() and host.converged
    for per_element, ref in ((True, per), (False, both)):
        for k in (1, 7):
            assert _same(moda_amd.iterative_closest_point_device(xt, yt, per_element=per_element, check_every=k), ref)


def test_graph_capture_replays_the_eager_bits():
    """check_every = 0: the captured call, replayed on fresh inputs, gives the eager bits.  (That the graph is a chain is a
    property of the code -- every launch goes to the current stream -- and is not inspected here: DESIGN, f3c-seq.)"""
    X, Y = stopping_batch()
    lens = I32([1500, 1400, 1300])
    sx, sy = T(X).clone(), T(Y).clone()
    kw = dict(per_element=True, max_iterations=30, check_every=0)
    moda_amd.iterative_closest_point_device(sx, sy, lens, **kw)              # loads the library before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sol = moda_amd.iterative_closest_point_device(sx, sy, lens, **kw)
    for shift in (0.0, 0.01):
        x2, y2 = T(X[::-1].copy()) + shift, T(Y[::-1].copy())
        sx.copy_(x2)
        sy.copy_(y2)
        g.replay()
        torch.cuda.synchronize()
        eager = moda_amd.iterative_closest_point_device(x2, y2, lens, **kw)
        assert _same(sol, eager) and torch.equal(sol.idx, eager.idx)
    assert sol.converged.any()


def _raw_metrics(d1, d2, lens, bbox):
    B, Mm, N = d1.shape[0], d1.shape[1], d2.shape[1]
    out = torch.full((B, 10), -1.0, dtype=torch.float64, device=DEV)
    _lib.call("moda_seq_metrics", _lib.ptr(d1), _lib.ptr(d2), B, Mm, N, _lib.ptr(lens), _lib.ptr(bbox), _lib.ptr(out), _lib.stream())
    return out.cpu().numpy()


def test_seq_metrics_match_oracle():
    """moda_seq_metrics alone, on given squared distances: ragged and y_len == NULL, all ten columns.  Bars: a count differs from
    the float64 count only through distances within 5 u of the fp32-rounded threshold (n1 of G, n2 of V), so a precision is off
    by at most n / size + u (its one rounding), an F-score by 2 (n1 / G + n2 / V) + 8 u; cd is fp32 square roots (u / 2 each)
    averaged in float64: 2 u relative.  More than one 256-lane pass, odd lengths, and a frame of a single valid row."""
    rng = np.random.default_rng(21)
    bbox = np.array([1.0, 0.7, 1.3], np.float32)
    Mm, N, lens = 1501, 1027, (1501, 777, 1)
    # distances spread around the three thresholds of each frame, so every F-score is cut through
    d1 = (rng.uniform(0, 0.08, (3, Mm)) * bbox[:, None].astype(np.float64)).astype(np.float32) ** 2
    d2 = (rng.uniform(0, 0.08, (3, N)) * bbox[:, None].astype(np.float64)).astype(np.float32) ** 2
    d1[1, 5], d2[2, 7] = 0.0, 0.0
    poisoned = d1.copy()
    for b, n in enumerate(lens):
        poisoned[b, n:] = 0.0                                                 # padding under every threshold: it must not count
    for y_len, src in ((lens, poisoned), (None, d1)):
        got = _raw_metrics(T(src), T(d2), None if y_len is None else I32(y_len), T(bbox))
        for b in range(3):
            n = Mm if y_len is None else y_len[b]
            want, thresholds = icn.metrics_row(src[b, :n], d2[b], float(bbox[b]))
            assert abs(got[b, 0] - want[0]) <= 2 * U * want[0]
            cut = 0
            for k, thr in enumerate(thresholds):
                n1 = int((np.abs(src[b, :n].astype(np.float64) - thr) <= 5 * U * thr).sum())
                n2 = int((np.abs(d2[b].astype(np.float64) - thr) <= 5 * U * thr).sum())
                assert abs(got[b, 4 + 2 * k] - want[4 + 2 * k]) <= n1 / n + U
                assert abs(got[b, 5 + 2 * k] - want[5 + 2 * k]) <= n2 / N + U
                assert abs(got[b, 1 + k] - want[1 + k]) <= 2 * (n1 / n + n2 / N) + 8 * U
                cut += 0 < want[5 + 2 * k] < 1
            assert cut >= 2
    zero = _raw_metrics(T(np.full((1, 4), 9.0, np.float32)), T(np.full((1, 3), 9.0, np.float32)), None, T(np.ones(1, np.float32)))
    assert (zero[0, 1:] == 0).all() and zero[0, 0] == 6.0                     # 0 / 0 is 0


@functools.lru_cache(maxsize=None)
def _sequence():
    shape = (40, 40, 40)
    gts = [M.TriMesh(*M.marching_cubes(T(_sphere(shape, r, o)), 0.0)) for r, o in
           ((14.0, (0.137, 0.071, -0.053)), (13.0, (-0.21, 0.33, 0.12)), (15.0, (0.4, -0.15, 0.27)))]
    pred = M.marching_cubes(T(_sphere(shape, 14.0 * 1.02, (0.537, -0.229, 0.047))), 0.0)[0]
    # one mesh in three poses, as a warped rest mesh is: the same V in every frame
    shifts = torch.tensor([[0.0, 0.0, 0.0], [0.11, 0.05, -0.02], [-0.07, 0.02, 0.06]], device=DEV)
    verts = (pred[None] * torch.tensor([1.0, 13.0 / 14.0, 15.0 / 14.0], device=DEV)[:, None, None] + shifts[:, None]).contiguous()
    return verts, gts


def test_eval_sequence_matches_eval_mesh_and_oracle():
    verts, gts = _sequence()
    lens = [len(g.vertices_t) for g in gts]
    assert len(set(lens)) == 3
    seq = moda_amd.eval_sequence(verts, gts)
    frames, _ = icn.eval_sequence(verts.cpu().numpy(), [g.vertices_t.cpu().numpy() for g in gts])
    got = {k: getattr(seq, k).cpu().numpy() for k in ("cd", "f001", "f002", "f005", "fitted_scale", "bbox_max")}
    rows = seq.metrics.cpu().numpy()
    assert seq.verts.shape == verts.shape and seq.iterations.shape == (3,) and seq.converged.dtype == torch.bool
    for f in range(3):
        one = moda_amd.eval_mesh(verts[f], gts[f])
        want = frames[f]
        G, V = len(want["d_gt"]), len(want["d_back"])
        print("frame", f, "G", G, "V", V, "iterations", int(seq.iterations[f]), len(one["icp"].t_history), len(want["icp"].t_history),
              "cd", got["cd"][f], one["cd"], want["cd"], "f", [(got[k][f], one[k], want[k]) for k in ("f001", "f002", "f005")])
        assert abs(got["bbox_max"][f] - one["bbox_max"]) <= 4 * U * one["bbox_max"]
        assert abs(got["bbox_max"][f] - want["bbox_max"]) <= 4 * U * want["bbox_max"]
        assert abs(got["fitted_scale"][f] - one["fitted_scale"]) <= 4 * U * abs(one["fitted_scale"])
        assert abs(got["fitted_scale"][f] - want["fitted_scale"]) <= 4 * U * abs(want["fitted_scale"])
        for k in range(3):                                                    # the precision pairs: counts over sizes
            thr = want["thresholds"][("f001", "f002", "f005")[k]]
            n1 = int((np.abs(want["d_gt"] - thr) <= 5 * U * thr).sum())
            n2 = int((np.abs(want["d_back"] - thr) <= 5 * U * thr).sum())
            assert abs(rows[f, 4 + 2 * k] - want["row"][4 + 2 * k]) <= n1 / G + U
            assert abs(rows[f, 5 + 2 * k] - want["row"][5 + 2 * k]) <= n2 / V + U
        assert abs(got["cd"][f] - one["cd"]) <= 1e-5 * one["cd"] and abs(got["cd"][f] - want["cd"]) <= 1e-5 * want["cd"]
        for key in ("f001", "f002", "f005"):
            thr = want["thresholds"][key]
            n1 = int((np.abs(want["d_gt"] - thr) <= 5 * U * thr).sum())
            n2 = int((np.abs(want["d_back"] - thr) <= 5 * U * thr).sum())
            bound = 2 * (n1 / G + n2 / V) + 8 * U
            assert abs(got[key][f] - one[key]) <= bound and abs(got[key][f] - want[key]) <= bound
    assert any(0 < frames[f][k] < 1 for f in range(3) for k in ("f001", "f002", "f005"))
    s = seq.summary()
    assert s["cd_ave"] == pytest.approx(got["cd"].mean(), rel=1e-14) and s["cd_max"] == got["cd"].max()
    for key in ("f001", "f002", "f005"):
        assert s[key + "_ave"] == pytest.approx(got[key].mean(), rel=1e-14) and s[key + "_min"] == got[key].min()
    # a padded tensor with lengths (the padding holds a vertex of the prediction: it would win if it were read) == the list
    padded = verts[:, :1].expand(3, max(lens), 3).clone()
    for f, g in enumerate(gts):
        padded[f, :lens[f]] = g.vertices_t
    for other in (moda_amd.eval_sequence(verts, padded, gt_lens=lens), moda_amd.eval_sequence(verts, gts)):   # and a second run
        assert torch.equal(other.metrics, seq.metrics) and torch.equal(other.verts, seq.verts)
        assert torch.equal(other.iterations, seq.iterations) and torch.equal(other.fitted_scale, seq.fitted_scale)


def test_refusals():
    x, y = T(np.random.default_rng(1).uniform(-1, 1, (2, 10, 3)).astype(np.float32)), \
        T(np.random.default_rng(2).uniform(-1, 1, (2, 12, 3)).astype(np.float32))
    icp, ev = moda_amd.iterative_closest_point_device, moda_amd.eval_sequence
    with pytest.raises(ValueError, match="empty"):
        icp(x, y[:, :0])
    with pytest.raises(ValueError, match="empty"):
        icp(x[:, :0], y)
    with pytest.raises(ValueError, match="empty"):
        ev(x, [y[0], y[1][:0]])
    for bad in ([0, 3], [3, 13], [3], I32([3, 0])):
        with pytest.raises(ValueError, match="y_len"):
            icp(x, y, bad)
        with pytest.raises(ValueError, match="y_len"):
            ev(x, y, gt_lens=bad)
    with pytest.raises(ValueError):
        icp(x, y[:1])                                                         # batch sizes
    with pytest.raises(ValueError):
        ev(x, [y[0]])                                                         # frame counts
    with pytest.raises(ValueError):
        icp(x[0], y[0])                                                       # unbatched
    yb = y.clone()
    yb[1, 3, 0] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        icp(x, yb)
    icp(x, yb, [12, 3])                                                       # ... but not where it is padding
    with pytest.raises(RuntimeError):
        icp(x.cpu(), y.cpu())
    with pytest.raises(RuntimeError):
        ev(x.cpu(), y)
    with pytest.raises(NotImplementedError):
        icp(x.clone().requires_grad_(True), y)
    with pytest.raises(NotImplementedError):
        ev(x, y.clone().requires_grad_(True))
