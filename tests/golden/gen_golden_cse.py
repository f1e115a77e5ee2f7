"""Generate tests/golden/g34_cse.npz by running the reference's own resample_dp, bbox_dp2rnd, ood_check_cse, compute_flow_cse and
match2flo (nnutils/geom_utils.py) on the CPU (development container only, like gen_golden_frames.py), in fp32 and in float64
(torch's default dtype switched, since the reference's helpers allocate in the default dtype).  Inputs and outputs only.

Keys: `rs/names`, and per resample case `rs/<name>/feats|bbox|kaug|target` with the reference's `out32|out64` (and `n32|n64`, the
same through F.normalize(., 2, 1)) and `d2r32|d2r64` (bbox_dp2rnd); `ood/names`, per case `ood/<name>/feats|embed|dp_idx` with
`valid32|err32|valid64|err64|idx64`; `flow/names`, per case `flow/<name>/a|b|warp_a|warp_b|img_size` with `fa32|fb32|fa64|fb64`
and `ma64|mb64`; `nearest/<in>_<out>`: the row indices F.interpolate(mode='nearest') picks.

The fixtures' own preconditions are asserted here: every flow case (the "unique match" cases) has a float64 margin between best
and runner-up score above 8x the arg-max bound of tests/cse_numpy.py for every query in both directions, and in every ood case the
reference's fp32 arg-max indices equal its float64 ones.

    python tests/golden/gen_golden_cse.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import cse_numpy as O  # noqa: E402


def in_dtype(dt, fn, *args):
    torch.set_default_dtype(dt)
    try:
        return fn(*[torch.from_numpy(np.asarray(a)).to(dt) if isinstance(a, np.ndarray) and a.dtype.kind == 'f' else a for a in args])
    finally:
        torch.set_default_dtype(torch.float32)


def unit(rng, *shape):
    """Random features, L2-normalised over axis -3 (the channel axis of an image)."""
    f = rng.standard_normal(shape)
    return (f / np.linalg.norm(f, axis=-3, keepdims=True)).astype(np.float32)


def ref_indices(embed, feats, dt):
    """The arg-max of ood_check_cse's costmap expression in dtype dt."""
    e, f = torch.from_numpy(embed).to(dt), torch.from_numpy(feats).to(dt)
    N, (bs, _, h, w) = e.shape[0], f.shape
    return np.stack([(e.view(N, 16, 1) * f[i].view(1, 16, h * w)).sum(-2).argmax(-1).numpy() for i in range(bs)])


def main():
    _, _, geom, _ = _ref_import.import_reference()
    rng = np.random.default_rng(34)
    out = {}

    # ---- resample_dp -----------------------------------------------------------------------------------------------------
    f24 = (rng.standard_normal((2, 16, 24, 24)) * 0.5).astype(np.float32)
    f24[:, :, :3] = 0                                                     # rows outside the DensePose box are zero
    f5 = rng.standard_normal((2, 16, 5, 5)).astype(np.float32)
    kaug = np.asarray([[1.7, 1.6, 40.0, 60.0], [2.2, 2.1, 10.0, 25.0]], np.float32)
    inside = np.asarray([[42.0, 63.0, 137.0, 150.0], [8.0, 26.0, 131.0, 144.0]], np.float32)        # the crop covers the source
    outside = np.asarray([[30.0, 50.0, 137.0, 150.0], [20.0, 30.0, 131.0, 144.0]], np.float32)       # the crop reaches past the source
    mixed = np.asarray([[0.0, 0.0, 0.0, 0.0], [12.0, 27.0, 94.0, 105.0]], np.float32)
    zero = np.zeros((2, 4), np.float32)
    cases = [("zero_up", f5, zero, 7), ("zero_down", f24, zero, 10), ("grid", f24, inside, 12), ("outside", f24, outside, 12),
             ("mixed", f24, mixed, 8)]
    out["rs/f24"], out["rs/f5"], out["rs/kaug"] = f24, f5, kaug
    for name, feats, bbox, target in cases:
        out[f"rs/{name}/src"] = np.asarray("f5" if feats is f5 else "f24")
        out[f"rs/{name}/bbox"], out[f"rs/{name}/target"] = bbox, np.asarray(target)
        for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
            with np.errstate(all="ignore"):
                r = in_dtype(dt, geom.resample_dp, feats, bbox, kaug, target)
                out[f"rs/{name}/out{tag}"] = r.numpy()
                if name == "grid":
                    out[f"rs/{name}/n{tag}"] = F.normalize(r, 2, 1).numpy()
                out[f"rs/{name}/d2r{tag}"] = in_dtype(dt, geom.bbox_dp2rnd, bbox, kaug).numpy()
        live = out[f"rs/{name}/out64"][[i for i in range(2) if np.abs(bbox).sum() == 0 or np.abs(bbox[i]).sum() != 0]]
        print(name, "non-zero share", (live != 0).mean())
        assert (live != 0).mean() > 0.15, name                             # a fixture that samples the source, not only padding
    assert (out["rs/outside/out64"] == 0).mean() > 0.3
    out["rs/names"] = np.asarray([c[0] for c in cases])

    # ---- ood_check_cse ---------------------------------------------------------------------------------------------------
    names = []
    for name, h, N, H in (("w24", 24, 600, 48), ("w16", 16, 257, 16), ("w7", 7, 40, 5)):
        for attempt in range(50):
            feats = unit(rng, 3, 16, h, h)
            feats[:, :, : h // 4] = 0                                     # pixels outside the box normalise to zero
            embed = rng.standard_normal((N, 16))
            embed = (embed / np.linalg.norm(embed, axis=1, keepdims=True)).astype(np.float32)
            embed[N // 3] = -np.abs(embed[N // 3])                        # may tie at the zero pixels: first zero pixel
            i32, i64 = ref_indices(embed, feats, torch.float32), ref_indices(embed, feats, torch.float64)
            if (i32 == i64).all():
                break
        assert (i32 == i64).all(), name
        dp_idx = rng.integers(0, N, (3, H, H))
        dp_idx[rng.random((3, H, H)) < 0.4] = 0
        dp_idx[2] = 0                                                     # an empty mask: NaN and False
        if H % h == 0:                                                    # frame 0: a forward-backward consistent labelling (small error)
            lab = np.zeros(h * h, np.int64)
            lab[i64[0][::-1]] = np.arange(N)[::-1]                        # a pixel's label: the lowest row matched to it
            dp_idx[0] = np.repeat(np.repeat(lab.reshape(h, h), H // h, 0), H // h, 1)
        names.append(name)
        out[f"ood/{name}/feats"], out[f"ood/{name}/embed"], out[f"ood/{name}/dp_idx"] = feats, embed, dp_idx.astype(np.int32)
        out[f"ood/{name}/idx64"] = i64.astype(np.int32)
        for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
            v, e = in_dtype(dt, geom.ood_check_cse, feats, embed, torch.from_numpy(dp_idx))
            out[f"ood/{name}/valid{tag}"], out[f"ood/{name}/err{tag}"] = v.numpy(), e.numpy()
    out["ood/names"] = np.asarray(names)

    # ---- compute_flow_cse / match2flo ------------------------------------------------------------------------------------
    names = []
    for name, w in (("w16", 16), ("w24", 24)):
        for attempt in range(200):
            a, b = unit(rng, 16, w, w), unit(rng, 16, w, w)
            qa, qb = a.reshape(16, -1).T, b.reshape(16, -1).T
            s = O.scores64(qa, qb)
            if (O.margin(s) > 8 * O.argmax_bound(qa, qb)).all() and (O.margin(s.T) > 8 * O.argmax_bound(qb, qa)).all():
                break
        assert (O.margin(s) > 8 * O.argmax_bound(qa, qb)).all() and (O.margin(s.T) > 8 * O.argmax_bound(qb, qa)).all(), name
        warp_a = np.asarray([[3.1, 0, 41.0], [0, 2.9, 77.0], [0, 0, 1]], np.float32)
        warp_b = np.asarray([[2.6, 0, 65.0], [0, 3.3, 52.0], [0, 0, 1]], np.float32)
        img_size = 256
        names.append(name)
        out.update({f"flow/{name}/a": a, f"flow/{name}/b": b, f"flow/{name}/warp_a": warp_a, f"flow/{name}/warp_b": warp_b,
                    f"flow/{name}/img_size": np.asarray(img_size)})
        out[f"flow/{name}/ma64"], out[f"flow/{name}/mb64"] = O.argmax_rule(s).astype(np.int32), O.argmax_rule(s.T).astype(np.int32)
        for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
            keep = geom.match2coords                                      # its .float() is fp32 whatever the default dtype is
            if dt == torch.float64:
                geom.match2coords = lambda match, w_rszd: keep(match, w_rszd).double()
            try:
                fa, fb = in_dtype(dt, geom.compute_flow_cse, a, b, warp_a, warp_b, img_size)
            finally:
                geom.match2coords = keep
            out[f"flow/{name}/fa{tag}"], out[f"flow/{name}/fb{tag}"] = fa.numpy(), fb.numpy()
        # the reference's own matches agree with the oracle's rule (unique maxima)
        ca = torch.from_numpy(a).double(), torch.from_numpy(b).double()
        cost = (ca[1][:, None, None] * ca[0][..., None, None]).sum(0).view(w * w, w * w)
        assert (cost.max(1)[1].numpy() == out[f"flow/{name}/ma64"]).all() and (cost.max(0)[1].numpy() == out[f"flow/{name}/mb64"]).all()
    out["flow/names"] = np.asarray(names)

    # ---- the `nearest` index rule ----------------------------------------------------------------------------------------
    for inn, o in ((512, 112), (256, 112), (112, 112), (7, 5)):
        src = torch.arange(inn, dtype=torch.float32)[None, None, :, None].expand(1, 1, inn, inn).contiguous()
        out[f"nearest/{inn}_{o}"] = F.interpolate(src, (o, o), mode='nearest')[0, 0, :, 0].long().numpy().astype(np.int32)

    path = os.path.join(HERE, "g34_cse.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
