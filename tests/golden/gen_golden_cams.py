"""Generate tests/golden/g40_cams.npz by running the reference's own align_sim3, visual_hull_align, rtk_invert, rtk_compose and
rot_angle (nnutils/geom_utils.py) on seeded inputs, on the CPU (development container only, like the other generators; the heavy
imports are stubbed by _ref_import).  Inputs and outputs only.

Two shims, neither of which edits the reference:
  * visual_hull_align hands 0-d tensors to np.linspace, which under this numpy returns a tensor, and the call then fails on
    `.astype`.  For that call np.linspace (geom.np.linspace) is replaced by `lambda a, b, n: np.linspace(float(a), float(b), n)`,
    the float64 evaluation older numpy performed, and put back afterwards.
  * the function returns the cameras only; to store which lattice points it selected, geom.F is replaced for that call by a
    namespace whose grid_sample is torch's own and keeps each chunk's result; the selection is then formed from them by the
    function's own two lines (`[:, 0, 0].sum(0)`, `> 0.8 * num_view`).

align_sim3 runs on float64 arrays whose rotations are orthogonal to float64 precision: scipy's Rotation.from_matrix first
projects a matrix that is not orthogonal onto the nearest rotation (an SVD), which moda_amd.cams and tests/cams_numpy.py do not
restate; for fp32-rounded rotations that step moves a quaternion entry by about 3e-9 (measured), far below fp32 resolution.
It writes its second argument and is_inlier in place, so copies go in and the entry the fallback set is read off the copy.

Hull scenes: binary masks put whole regions of the lattice EXACTLY on the threshold when 0.8 V is an integer (a point inside 4
of 5 discs scores 4), where fp32 and float64 cannot agree on `>`.  A scene is therefore redrawn (next seed) until at most 4
lattice points lie within 1e-4 of the threshold in float64 (tests/cams_numpy.py); the attempt that was kept is printed.

Keys: numpy_version, scipy_version; sim3/<case>/{a, b, inlier, err, out, inlier_after} (inlier absent: None was passed);
hull/<scene>/{rtk, kaug, masks (uint8), out (fp32), selected (packbits of 64^3), count}; rtk/{x, inv, y, comp} for rtk_invert(x, 3)
and rtk_compose(x, y); angle/{mat, out}.

    python tests/golden/gen_golden_cams.py
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402

SIM3_CASES = (("n1", 1, "none"), ("n2", 2, "none"), ("n7_some", 7, "some"), ("n40_none", 40, "none"), ("n40_allfalse", 40, "allfalse"),
              ("n40_all", 40, "all"), ("n65_some", 65, "some"), ("n65_wide", 65, "wide"))
HULL_SCENES = (("v3", 3, 16, 16, 0), ("v7", 7, 24, 40, 0), ("v12", 12, 32, 32, 0), ("v5", 5, 16, 16, 0), ("v10", 10, 20, 28, 0),
               ("v6_kaug", 6, 24, 24, 1), ("v5_long", 5, 16, 16, 2))


def rotations(rng, n, spread=None):
    """n rotation matrices: uniformly random (QR), or, with `spread`, rotations by up to `spread` radians about random axes."""
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    if spread is None:
        return q
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(*(spread if isinstance(spread, tuple) else (0, spread)), n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    rod = np.eye(3)[None] + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * np.matmul(K, K)
    return rod


def cams(R, t):
    out = np.tile(np.eye(4), (len(R), 1, 1))
    out[:, :3, :3], out[:, :3, 3] = R, t
    return out


def sim3_case(rng, n, kind):
    Ra = rotations(rng, n)
    delta = rotations(rng, 1)[0]
    noise = rotations(rng, n, spread=np.deg2rad(120.0 if kind == "wide" else 8.0))
    Rb = np.matmul(np.matmul(Ra, noise), delta.T)
    a = cams(Ra, rng.standard_normal((n, 3)) + [0, 0, 3])
    b = cams(Rb, 0.4 * (rng.standard_normal((n, 3)) + [0, 0, 3]))
    err = rng.uniform(0.1, 1.0, n).astype(np.float32)
    inl = {"none": None, "all": np.ones(n, bool), "allfalse": np.zeros(n, bool), "some": rng.uniform(size=n) < 0.4,
           "wide": None}[kind]
    if kind == "some":
        inl[0] = True
    return a, b, inl, err


def hull_scene(rng, V, h, w, variant):
    R = rotations(rng, V)
    t = np.zeros((V, 3))
    t[:, 2] = 3.0 + rng.uniform(-0.2, 0.2, V)
    rtk = cams(R, t).astype(np.float32).astype(np.float64)
    f = 1.2 * w
    kaug = np.tile(np.asarray([1.0, 1.0, 0.0, 0.0], np.float32), (V, 1))
    if variant == 1:                                                             # a crop: p = Kaug^-1 K P
        kaug = np.stack([rng.uniform(0.8, 1.25, V), rng.uniform(0.8, 1.25, V), rng.uniform(-3, 3, V), rng.uniform(-3, 3, V)], -1).astype(np.float32)
    rtk[:, 3] = [f, f, w / 2.0, h / 2.0]
    rtk = rtk.astype(np.float32)
    centre, radius = np.asarray([0.2, -0.1, 0.15]), 0.35
    pc = np.matmul(rtk[:, :3, :3].astype(np.float64), centre) + rtk[:, :3, 3]
    ka = kaug.astype(np.float64)
    fx, fy, px, py = f / ka[:, 0], f / ka[:, 1], (w / 2.0 - ka[:, 2]) / ka[:, 0], (h / 2.0 - ka[:, 3]) / ka[:, 1]
    u, v, rad = fx * pc[:, 0] / pc[:, 2] + px, fy * pc[:, 1] / pc[:, 2] + py, fx * radius / pc[:, 2]
    yy, xx = np.mgrid[:h, :w] + 0.5                                               # pixel centres in grid_sample's frame
    masks = ((xx[None] - u[:, None, None]) ** 2 + (yy[None] - v[:, None, None]) ** 2 <= rad[:, None, None] ** 2).astype(np.uint8)
    if variant == 2:
        rtk = np.concatenate([rtk, rtk[:2]])                                     # longer than V: the reference trims it
    return rtk, kaug, masks


def main():
    _, _, geom, _ = _ref_import.import_reference()
    import scipy
    out = {"numpy_version": np.asarray(np.__version__), "scipy_version": np.asarray(scipy.__version__)}
    sys.path.insert(0, os.path.dirname(HERE))
    import cams_numpy
    rng = np.random.default_rng(40)
    for name, n, kind in SIM3_CASES:
        a, b, inl, err = sim3_case(rng, n, kind)
        b_in, inl_in = b.copy(), None if inl is None else inl.copy()
        with contextlib.redirect_stdout(io.StringIO()):
            res = geom.align_sim3(a.copy(), b_in, is_inlier=inl_in, err_valid=err.copy())
        pre = "sim3/%s/" % name
        out[pre + "a"], out[pre + "b"], out[pre + "err"], out[pre + "out"] = a, b, err, res
        if inl is not None:
            out[pre + "inlier"], out[pre + "inlier_after"] = inl, inl_in
        print(name, n, kind, "fallback set", None if inl is None else np.nonzero(inl_in != inl)[0].tolist())
    real_linspace, real_F = np.linspace, geom.F
    for name, V, h, w, variant in HULL_SCENES:
        for attempt in range(50):
            rtk, kaug, masks = hull_scene(np.random.default_rng([40, len(name), V, attempt]), V, h, w, variant)
            s64 = cams_numpy.hull_scores(rtk, kaug, masks, 64)[0]
            if int((np.abs(s64 - 0.8 * V) < 1e-4).sum()) <= 4:
                break
        else:
            raise SystemExit("no scene for " + name)
        kept = []

        def grid_sample(*args, **kw):
            kept.append(real_F.grid_sample(*args, **kw))
            return kept[-1]
        try:
            geom.np.linspace = lambda a, b, n: real_linspace(float(a), float(b), n)
            geom.F = types.SimpleNamespace(grid_sample=grid_sample)
            with contextlib.redirect_stdout(io.StringIO()) as said:
                res = geom.visual_hull_align(rtk.copy(), kaug.copy(), masks.astype(np.float32))
        finally:
            geom.np.linspace, geom.F = real_linspace, real_F
        score = torch.cat([k[:, 0, 0].sum(0) for k in kept])
        sel = (score > 0.8 * V).numpy()
        pre = "hull/%s/" % name
        out[pre + "rtk"], out[pre + "kaug"], out[pre + "masks"], out[pre + "out"] = rtk, kaug, masks, res.numpy()
        out[pre + "selected"], out[pre + "count"] = np.packbits(sel), np.int64(sel.sum())
        print(name, (V, h, w), "attempt", attempt, "selected", int(sel.sum()), "|", said.getvalue().strip().splitlines()[-1])
    x, y = rng.standard_normal((2, 5, 3, 12))
    x[..., :9] = rotations(rng, 15).reshape(5, 3, 9)
    y[..., :9] = rotations(rng, 15).reshape(5, 3, 9)
    out["rtk/x"], out["rtk/y"] = x, y
    out["rtk/inv"] = geom.rtk_invert(torch.from_numpy(x).reshape(5, 36), 3).numpy()
    out["rtk/comp"] = geom.rtk_compose(torch.from_numpy(x), torch.from_numpy(y)).numpy()
    # angles where fp32 acos is good to 1e-6: its error is eps / sin(angle), so neither the clamp at 1 - 1e-4 nor angles near pi
    mats = np.concatenate([rotations(rng, 20, spread=(0.3, 2.8)), rotations(rng, 12, spread=(0.5, 2.6))]).astype(np.float32)
    out["angle/mat"], out["angle/out"] = mats, geom.rot_angle(torch.from_numpy(mats)).numpy()
    path = os.path.join(HERE, "g40_cams.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
