"""CPU: the float64 reference of the correspondence heads and per-ray sums (tests/corresp_numpy.py) against float64 autograd through
oracle/torch_ref.py::project and through torch restatements of vrender_flo / compute_pts_exp / the other four, against flo_coarse,
flo_valid (tests/golden/g10_corresp_*.npz) and pts_exp (tests/golden/g11_heads_*.npz); the case builder tests/test_gpu_corresp.py
runs on the device; the conditions those cases must meet for its per-element bars to mean something; and the fp32 models of the
kernels held to the same bars, as written and with five seeded mistakes.

Cases: (S, N) in SN -- S = 1, 2, one short of / at / one past one and two lane trips, 200 (four trips, the last partial); N = 9, 5, 1
rays, never a multiple of the four waves of a workgroup.  img_size 512 (S even) and 300 (S odd).
  project  Kinv with distinct focal entries 1 / 400 ... 1 / 700, a principal point of 200 ... 300 pixels and junk in the entries
           mat2K drops.  front: Z in [0.5, 5].  grazing: |1e-6 + Z| log-uniform in [1e-3, 0.5], both signs, the first sample of a
           ray at 1e-3.
  flow     projections inside 0.9 img_size of the origin and Z in [0.5, 5] (valid), weights >= 0 adding up to 1.
           mixed: per ray a prefix invalid by depth / by norm, runs straddling sample 64 by depth / norm / both, every other
           sample, ONE sample that is not lane 0's (what catches `ninv` read from lane 0), sample 64 alone, none.
           edge: Z = 1e-5f (valid), its fp32 neighbours (below: invalid), (u, v) = (2 img_size, 0) (valid), nextafter of it
           (invalid).  all_invalid: every ray but the last.  single_valid: one valid sample per ray.  poison: NaN, Inf, -Inf in
           w, u, v at samples invalid by depth.
  pts_exp  soft / one-hot / all-zero weights (every ray but the last).
  points   o, d, sorted depths.     rows  (F, k, C): k = 1 ... 16, C below / at / past one and two column blocks of 64.
  vis      (n_neg, n_pos): n_neg odd (the second launch reads from an address 4 bytes off any 8-byte boundary), one element, one
           past a workgroup.
Output gradients have one sign per (ray, channel) and magnitudes in [0.25, 1]: a sum over the samples of a ray is then of the size of
its terms, and the condition asserted here -- outside `grazing`, no element's bound FLOOR u condition exceeds 1e-4 of the largest
magnitude of its ray's elements -- holds with room.  Rows that cancel as a whole are left out of that assertion (they are still held
to their bar): an all-invalid or all-zero ray, and d_w of a ray with ONE live sample, where (g . (xy - o)) / den + common is the
regulariser's residue 1e-9 / w of either term.

Seeded mistakes (corresp_numpy.MUTATIONS), each caught by the bar of the GPU test on the fp32 model:
  one_trip     lanes stop after their first trip           every sum at every S > 64: d_rtk / flo / pts_exp / d_o, d_d; first at
                                                           S = 65 (project front, flow valid, pts_exp soft, points); S <= 64 is
                                                           unchanged bit for bit
  flow_common  `common` dropped from the flow backward     d_w of flow valid, every S >= 2
  pts_common   `common` dropped from pts_exp's backward    d_w_pts of pts_exp soft, every S >= 2
  den_sq       (den * den) written as den in dZ            d_xyz and d_rtk of project front, every S
  ninv_wave    ninv not summed across the wave             `valid` of flow mixed (ray 6: its one invalid sample is not lane 0's), S >= 2"""
import functools

import numpy as np
import pytest
import torch

import corresp_numpy as cn
from oracle import torch_ref as tr
from moda_amd import synth
from helpers import golden, rel_err
from test_torch_ref import torch_scene, torch_scene_heads, g11_rays

SN = ((1, 9), (2, 9), (63, 9), (64, 9), (65, 9), (128, 9), (129, 9), (200, 9), (65, 5), (129, 1), (200, 5))
KINDS = {"project": ("front", "grazing"), "flow": ("valid", "mixed", "edge", "all_invalid", "single_valid", "poison"),
         "pts_exp": ("soft", "onehot", "zero"), "points": ("rays",)}
ROWS_CASES = ((5, 1, 3), (5, 2, 3), (7, 3, 21), (3, 5, 64), (4, 9, 65), (2, 16, 130))
VIS_CASES = ((1, 3), (5, 9), (255, 300), (257, 256), (777, 1100))
BOUND_CAP = 1e-4
f32 = lambda a: np.ascontiguousarray(a, np.float32)


def img_of(S):
    return 512.0 if S % 2 == 0 else 300.0


def _biased(rng, shape):
    """One sign per (ray, channel), magnitudes in [0.25, 1]."""
    sign = np.where(rng.uniform(size=(shape[0],) + (1,) * (len(shape) - 2) + (shape[-1],)) < 0.5, -1.0, 1.0)
    return f32(rng.uniform(0.25, 1.0, shape) * sign)


def _weights(rng, N, S):
    w = rng.uniform(size=(N, S)) ** 3
    return f32(w / w.sum(-1, keepdims=True))


def _run(S, lo, hi):
    m = np.zeros(S, bool)
    m[min(lo, S - 1):min(hi, S)] = True
    return m


def _project_case(rng, kind, S, N):
    R = np.linalg.qr(rng.normal(size=(N, 3, 3)))[0]
    xyz = rng.uniform(-0.2, 0.2, (N, S, 3))
    T = np.stack([rng.uniform(-0.3, 0.3, N), rng.uniform(-0.3, 0.3, N), rng.uniform(0.85, 4.65, N)], -1)
    if kind == "grazing":
        T[:, 2] = rng.uniform(-0.2, 0.2, N)
        den = 10.0 ** rng.uniform(-3.0, np.log10(0.5), (N, S)) * np.where(rng.uniform(size=(N, S)) < 0.5, -1.0, 1.0)
        den[:, 0] = np.where(np.arange(N) % 2 == 0, 1e-3, -1e-3)
        Z = (xyz * R[:, None, 2, :]).sum(-1) + T[:, None, 2]
        xyz = xyz + R[:, None, 2, :] * (den - 1e-6 - Z)[..., None]
    rtk = np.zeros((N, 21))
    rtk[:, :9], rtk[:, 9:12] = R.reshape(N, 9), T
    k0, k1 = 1.0 / rng.uniform(400, 700, N), 1.0 / rng.uniform(400, 700, N)
    rtk[:, 12], rtk[:, 16], rtk[:, 14], rtk[:, 17] = k0, k1, -rng.uniform(200, 300, N) * k0, -rng.uniform(200, 300, N) * k1
    rtk[:, [13, 15, 18, 19]] = 0.01 * rng.normal(size=(N, 4))         # what mat2K drops: no output and no gradient
    rtk[:, 20] = 1.0
    return dict(xyz=f32(xyz), rtk=f32(rtk), g=_biased(rng, (N, S, 3)))


EDGE_Z = np.float32(cn.C5)


def _flow_case(rng, kind, S, N):
    img = img_of(S)
    proj = np.concatenate([rng.uniform(-0.9, 0.9, (N, S, 2)) * img, rng.uniform(0.5, 5.0, (N, S, 1))], -1).astype(np.float32)
    w = _weights(rng, N, S)
    depth = np.zeros((N, S), bool)
    norm = np.zeros((N, S), bool)
    r = lambda i: i % N
    if kind in ("mixed", "poison"):
        depth[r(0), :min(5, S)] = True
        (depth if kind == "poison" else norm)[r(1), :max(S // 2, 1)] = True
        depth[r(2)] |= _run(S, 60, 68)
        (depth if kind == "poison" else norm)[r(3)] |= _run(S, 62, 66)
        depth[r(4)] |= _run(S, 60, 70)
        if kind == "mixed":
            norm[r(4)] |= _run(S, 58, 66)
        depth[r(5), ::2] = True
        if N > 6 and S > 1:
            s6 = min(S - 1, 70)                                        # lane 6 of the second trip, or the last lane in use ...
            depth[6, s6 - (s6 % 64 == 0)] = True                       # ... but never lane 0 (S = 65: sample 63)
        if N > 7:
            (depth if kind == "poison" else norm)[7, min(S - 1, 64)] = True
    elif kind == "all_invalid":
        depth[:max(N - 1, 1), ::2] = True
        norm[:max(N - 1, 1), 1::2] = True
        depth[0] = True
    elif kind == "single_valid":
        depth[:, ::2] = True
        norm[:, 1::2] = True
        keep = (np.arange(N) * 29 + S - 1) % S
        depth[np.arange(N), keep] = norm[np.arange(N), keep] = False
    proj[..., 2][depth] = np.asarray([-0.3, 0.0, 1e-6, -1e-5], np.float32)[np.arange(int(depth.sum())) % 4]
    proj[..., 0][norm] = 3.0 * img
    if kind == "edge":
        up, dn = np.float32(np.inf), np.float32(-np.inf)
        edges = ((2, EDGE_Z), (2, np.nextafter(EDGE_Z, dn)), (2, np.nextafter(EDGE_Z, up)), (0, np.float32(2 * img)),
                 (0, np.nextafter(np.float32(2 * img), up)))
        for n in range(N):
            for j, (col, val) in enumerate(edges):
                for base in (0, 60):
                    s = (base + 13 * j + n) % S
                    proj[n, s] = (abs(proj[n, s, 0]), abs(proj[n, s, 1]), proj[n, s, 2])
                    proj[n, s, col] = val
                    if col == 0:
                        proj[n, s, 1] = 0.0
    c = dict(w=w, proj=proj, xys=f32(rng.uniform(0, img, (N, 2))), img=img, g=_biased(rng, (N, 2)))
    if kind == "poison":
        bad = np.asarray([np.nan, np.inf, -np.inf], np.float32)
        c["clean"] = dict(c, w=w.copy(), proj=proj.copy())
        k = np.arange(int(depth.sum()))
        w[depth] = bad[k % 3]
        proj[..., 0][depth] = bad[(k + 1) % 3]
        proj[..., 1][depth] = bad[(k // 3) % 3]
    return c


def _pts_case(rng, kind, S, N):
    w = _weights(rng, N, S)
    if kind == "onehot":
        w[:] = 0.0
        w[np.arange(N), (np.arange(N) * 37 + S - 1) % S] = 1.0
    if kind == "zero":
        w[:max(N - 1, 1)] = 0.0
    pts = rng.uniform(-0.2, 0.2, (N, 1, 3)) + rng.uniform(-0.1, 0.1, (N, S, 3))
    return dict(w=w, pts=f32(pts), g=_biased(rng, (N, 3)))


def _points_case(rng, kind, S, N):
    return dict(o=f32(rng.uniform(-1, 1, (N, 3))), d=f32(rng.normal(size=(N, 3))), z=f32(np.sort(rng.uniform(0.1, 6.0, (N, S)), -1)),
                g=_biased(rng, (N, S, 3)))


BUILDERS = {"project": _project_case, "flow": _flow_case, "pts_exp": _pts_case, "points": _points_case}


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return c


@functools.lru_cache(maxsize=None)
def case(op, kind, S, N):
    """One case of a per-ray operation: its inputs by corresp_numpy.OPS' names and 'g', the gradient of its output.  Read-only."""
    rng = np.random.default_rng(5100 + 977 * list(BUILDERS).index(op) + 131 * KINDS[op].index(kind) + 7 * S + N)
    return _freeze(BUILDERS[op](rng, kind, S, N))


@functools.lru_cache(maxsize=None)
def rows_case(F, k, C):
    rng = np.random.default_rng(6100 + 100 * F + 10 * k + C)
    return _freeze(dict(x=f32(rng.normal(size=(F, C))), k=k, g=f32(rng.normal(size=(F * k, C)))))


@functools.lru_cache(maxsize=None)
def vis_case(n_neg, n_pos):
    rng = np.random.default_rng(6200 + n_neg + 3 * n_pos)
    return _freeze(dict(x=f32(3.0 * rng.normal(size=(n_neg + n_pos,))), w_pos=f32(rng.uniform(0, 1, (n_pos,))), n_neg=n_neg,
                        g=f32(rng.uniform(0.5, 1.5, (1,)))))


def all_cases(op):
    """-> [(tag, case)] of one operation."""
    if op == "rows":
        return [((op, "rows") + c, rows_case(*c)) for c in ROWS_CASES]
    if op == "vis":
        return [((op, "vis") + c, vis_case(*c)) for c in VIS_CASES]
    return [((op, kind, S, N), case(op, kind, S, N)) for kind in KINDS[op] for S, N in SN]


_REFS = {}


def reference(op, tag, c):
    """corresp_numpy.reference of one case; computed once, shared, not to be modified."""
    if tag not in _REFS:
        _REFS[tag] = cn.reference(op, c)
    return _REFS[tag]


def figures(got, ref):
    return {k: float(cn.ratio(got[k], r[0], r[1]).max()) for k, r in ref.items()}


# ------------------------------------------------------------------------------------------------------------ vetting the reference
@pytest.mark.parametrize("op", list(cn.OPS))
def test_closed_forms_equal_float64_autograd_through_the_restatement(op):
    """Forward and every gradient, per element, to 1e-9 of what the element's own cancellation allows (the condition is the sum of
    its terms' magnitudes); where the condition is 0 both are exactly 0.  The poisoned cases too: torch.where lets nothing through."""
    names, diff, outs, fwd, grads, _, cond, _ = cn.OPS[op]
    for tag, c in all_cases(op):
        args = [c[k] for k in names]
        want = cn.torch_grads(op, c, torch.float64)
        got, cd = grads(*args, c["g"]), cond(*args, c["g"])
        for k in outs + tuple(diff.values()):
            assert got[k].shape == want[k].shape, (tag, k)
            assert np.isfinite(got[k]).all() and np.isfinite(want[k]).all(), (tag, k)
            assert (np.abs(got[k] - want[k]) <= 1e-9 * cd[k]).all(), (tag, k, float(np.abs(got[k] - want[k]).max()))
            assert cn.FLOOR[k] == 0 or (np.abs(want[k]) <= cd[k] * (1 + 1e-9)).all(), (tag, k)     # (FLOOR 0: a copy, exact)


def test_project_equals_float64_autograd_through_torch_ref():
    for tag, c in all_cases("project"):
        xyz, rtk = (torch.from_numpy(np.array(c[k])).double().requires_grad_(True) for k in ("xyz", "rtk"))
        out = tr.project(xyz, rtk)
        (out * torch.from_numpy(np.array(c["g"])).double()).sum().backward()
        got, cd = cn.project_grads(c["xyz"], c["rtk"], c["g"]), cn.project_condition(c["xyz"], c["rtk"], c["g"])
        for k, want in (("proj", out.detach()), ("d_xyz", xyz.grad), ("d_rtk", rtk.grad)):
            assert (np.abs(got[k] - want.numpy()) <= 1e-9 * cd[k]).all(), (tag, k)


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_flow_reference_reproduces_the_g10_golden(mode):
    """flo_coarse and flo_valid of the reference's own run: weights and canonical points from the torch restatement of the render
    pass, warped to the target frame (neu_dbs, backward=False) and projected with rtk_vec_target by corresp_numpy.project."""
    g = golden("g10_corresp_" + mode)
    N, S, B = 48, 12, 25
    m = torch_scene(10, B, True, perturb_bones=True)
    T = torch.from_numpy
    rays = {k: T(v) for k, v in synth.make_rays(10, N, B, rays_per_frame=8).items()}
    rays.update({k: T(v) for k, v in synth.make_corresp_rays(10, N, B, rays_per_frame=8).items()})
    with torch.no_grad():
        res = tr.render_rays(m, rays, S)
        xyz_t = tr.forward_warp(m, res["xyz_canonical_vis"], rays["bone_rts_target"])
    proj = cn.project(xyz_t.numpy(), rays["rtk_vec_target"].numpy())["proj"]
    out = cn.flow(res["weights"].numpy(), proj, rays["xys"].numpy().reshape(N, 2), 512.0)
    assert rel_err(out["flo"], g["flo_coarse"]) < 2e-4, rel_err(out["flo"], g["flo_coarse"])
    assert np.array_equal(out["valid"], g["flo_valid"].reshape(N, 1))


@pytest.mark.parametrize("mode", ["eval_ot", "train_ot"])
def test_pts_exp_reference_reproduces_the_g11_golden(mode):
    g = golden("g11_heads_" + mode)
    m = torch_scene_heads(11, 25)
    with torch.no_grad():
        res = tr.render_rays(m, g11_rays(), 12)
    out = cn.pts_exp(res["weights"].numpy(), res["xyz_canonical_vis"].numpy())["pts_exp"]
    assert rel_err(out, g["pts_exp"]) < 2e-4, rel_err(out, g["pts_exp"])


# ---------------------------------------------------------------------------------------------------------- conditions on the cases
def test_invalid_masks_agree_between_float32_and_float64_and_hold_what_the_kinds_promise():
    seen = set()
    for (op, kind, S, N), c in all_cases("flow"):
        m64, m32 = cn.invalid_mask(c["proj"], c["img"]), cn.invalid_mask(c["proj"], c["img"], np.float32)
        assert np.array_equal(m64, m32), (kind, S, N)
        live = (~m64).sum(-1)
        if kind == "valid":
            assert not m64.any()
        if kind == "all_invalid":
            assert live[0] == 0 and (N == 1 or live[-1] == S)
        if kind == "single_valid":
            assert (live == 1).all()
        if kind == "mixed" and N == 9 and S >= 65:
            assert m64[6].sum() == 1 and not m64[6, ::64].any() and m64[7].sum() == 1 and m64[7, 64]
            assert m64[2, 63] and m64[2, 64] and not m64[8].any()
        if kind == "edge":
            Z, u = c["proj"][..., 2], c["proj"][..., 0]
            for val, inv in ((EDGE_Z, False), (np.nextafter(EDGE_Z, np.float32(-1)), True), (np.nextafter(EDGE_Z, np.float32(1)), False)):
                hit = (Z == val) & (np.abs(u) < 1.5 * c["img"])                     # (S = 1: a later edge may sit on the same sample)
                seen.add(("z", inv, bool(hit.any())))
                assert (m64[hit] == inv).all(), (S, N, val)
            lim = np.float32(2 * c["img"])
            for val, inv in ((lim, False), (np.nextafter(lim, np.float32(np.inf)), True)):
                hit = (u == val) & (c["proj"][..., 1] == 0) & (Z >= EDGE_Z)
                seen.add(("u", inv, bool(hit.any())))
                assert (m64[hit] == inv).all(), (S, N, val)
        if kind == "poison":
            bad = ~np.isfinite(c["w"]) | ~np.isfinite(c["proj"]).all(-1)
            assert bad.any() and (c["proj"][..., 2][bad] < EDGE_Z).all() and np.isfinite(c["clean"]["w"]).all()
    assert {("z", False, True), ("z", True, True), ("u", False, True), ("u", True, True)} <= seen


@pytest.mark.parametrize("op", list(cn.OPS))
def test_bounds_stay_under_1e_4_of_the_rays_largest_magnitude(op):
    worst = {}
    for tag, c in all_cases(op):
        if tag[1] == "grazing":
            continue
        live = None                                                       # live samples of a ray, where the operation has weights
        if op == "flow":
            live = (~cn.invalid_mask(c["proj"], c["img"])).sum(-1)
        if op == "pts_exp":
            live = (np.asarray(c["w"]) != 0).sum(-1)
        for k, (truth, cond, of, bar) in reference(op, tag, c).items():
            t2, c2 = np.abs(truth).reshape(truth.shape[0], -1), cond.reshape(cond.shape[0], -1)
            top = t2.max(-1)
            cancels = np.zeros(top.shape, bool)                           # the rows that cancel as a whole (module docstring)
            if live is not None:
                cancels = (live <= 1) if k in ("d_w", "d_w_pts") else (live == 0)
            assert (top[~cancels] > 0).all() or not c2[~cancels].any(), (tag, k)
            rel = np.where(cancels[:, None], 0.0, cn.FLOOR[k] * cn.U * c2 / np.where(top > 0, top, 1.0)[:, None])
            worst[k] = max(worst.get(k, 0.0), float(rel.max()))
            assert rel.max() <= BOUND_CAP, (tag, k, float(rel.max()))
    print(f"corresp {op}: worst FLOOR u condition / ray's largest magnitude: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ the bars against a wrong kernel
@pytest.mark.parametrize("op", list(cn.OPS))
def test_fp32_model_of_the_kernel_stays_under_the_bar(op):
    names, diff, outs, fwd, grads, model, cond, _ = cn.OPS[op]
    worst = {}
    for tag, c in all_cases(op):
        ref = reference(op, tag, c)
        got = model(*[c[k] for k in names], c["g"])
        for k, f in figures(got, ref).items():
            w = worst.setdefault(k, [0.0, 0.0])
            w[0], w[1] = max(w[0], f), max(w[1], ref[k][2])
            assert f <= ref[k][3], (tag, k, f, ref[k][2])
        if op == "flow":
            assert np.array_equal(got["valid"], cn.flow(c["w"], c["proj"], c["xys"], c["img"])["valid"]), tag
    print(f"corresp {op}: fp32 model / float32 reference, worst |x - truth| / (u condition): "
          + ", ".join(f"{k} {v[0]:.2f} / {v[1]:.2f}" for k, v in worst.items()))


def _caught(op, tag, c, mutate):
    """The outputs of one case on which the mutated model misses the GPU test's assertions."""
    names = cn.OPS[op][0]
    got = cn.OPS[op][5](*[c[k] for k in names], c["g"], mutate=mutate)
    ref = reference(op, tag, c)
    bad = {k for k, f in figures(got, ref).items() if f > ref[k][3]}
    if op == "flow" and not np.array_equal(got["valid"], cn.flow(c["w"], c["proj"], c["xys"], c["img"])["valid"]):
        bad.add("valid")
    return bad


def _one(op, kind, S, N=9):
    return (op, kind, S, N), case(op, kind, S, N)


def test_lanes_that_stop_after_their_first_trip_are_caught():
    sums = {"project": ("front", {"d_rtk"}), "flow": ("valid", {"flo", "d_w", "d_proj"}), "pts_exp": ("soft", {"pts_exp", "d_w_pts", "d_pts"}),
            "points": ("rays", {"d_o", "d_d"})}
    for op, (kind, outs) in sums.items():
        for S, N in SN:
            bad = _caught(op, *_one(op, kind, S, N), "one_trip")
            assert bad == (outs if S > 64 else set()), (op, S, N, bad)


def test_a_dropped_common_term_is_caught():
    for S, N in SN:
        if S >= 2:
            assert _caught("flow", *_one("flow", "valid", S, N), "flow_common") == {"d_w"}, S
            assert _caught("pts_exp", *_one("pts_exp", "soft", S, N), "pts_common") == {"d_w_pts"}, S


def test_den_for_den_squared_in_projects_dz_is_caught():
    for S, N in SN:
        assert _caught("project", *_one("project", "front", S, N), "den_sq") == {"d_xyz", "d_rtk"}, S


def test_ninv_read_from_lane_0_is_caught():
    for S in (2, 63, 64, 65, 128, 129, 200):
        assert _caught("flow", *_one("flow", "mixed", S), "ninv_wave") == {"valid"}, S
