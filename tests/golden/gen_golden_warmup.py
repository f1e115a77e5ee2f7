"""Generate tests/golden/g36_warmup.npz by running the reference's own shape_init_loss, rtk_loss and compute_root_sm_loss
(nnutils/loss_utils.py) on the CPU, in fp32 and in float64, values and gradients (development container only, like
gen_golden_frame_pairs.py).  Inputs and outputs only.

shape_init_loss hard-codes 10 000 samples and draws them itself.  Here the module's `torch` is a proxy whose `rand` draws
(1, NSAMPLE, 3) instead -- with torch's own generator, recorded as `u` -- so the record stays small; everything else of the call
is the reference's.  Where trimesh is absent, `trimesh.Trimesh(...)`, which the reference constructs and never reads, is a stub that
accepts its arguments (the stub of _ref_import.py takes none).
The network's output y is taken by a forward hook, with its gradient dy; the targets themselves are local to the reference's
function, so they are pinned through dy = -2 (-y - dis) / N.

matrix_to_quaternion has no reference run behind it (pytorch3d is absent): nothing of it is recorded here.

Keys: shape/pts (V,3), shape/bound_factor, shape/w/<parameter> (the seeded NeRF(D=5, W=64, in_channels_xyz=63)), and per mode m in
(ellips, sphere) and precision p in (f32, f64): shape/<m>/u (NSAMPLE,3) fp32, shape/<m>/<p>/pts_samp, y, dy, loss, and for ellips
shape/ellips/<p>/d/<parameter> (None-gradient parameters are left out).  rtk/pred, rtk/raw (T,4,4) and rtk/<p>/total, rot_loss,
trn_loss, d_total, d_rot (gradients of the total and of rot_loss alone).  sm/rtk (T,4,4), sm/data_offset, sm/<p>/loss, d.

    python tests/golden/gen_golden_warmup.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import warmup_numpy as O  # noqa: E402

NSAMPLE = 300
V = 50
BOUND_FACTOR = 2 * 1.2
RTK_T = 37
SM_OFFSET = (0, 1, 3, 6, 40)


class TorchProxy:
    """`torch` for the reference's loss_utils: rand draws NSAMPLE points and records them; everything else is torch."""

    def __init__(self):
        self.u = None

    def rand(self, *shape, **kw):
        assert tuple(shape) == (1, 10000, 3), shape
        self.u = torch.rand(1, NSAMPLE, 3, **kw)
        return self.u

    def __getattr__(self, name):
        return getattr(torch, name)


def install_trimesh():
    """Only when trimesh is absent: a real installation is used as it is."""
    try:
        import trimesh  # noqa: F401
        return
    except ImportError:
        pass
    tm = types.ModuleType("trimesh")
    tm.Trimesh = type("Trimesh", (), {"__init__": lambda self, *a, **k: None})
    sys.modules["trimesh"] = tm


def poses(rng, T, spread):
    """(T,4,4) fp32: a smooth walk of rotations and translations, row 3 an intrinsics row."""
    out = np.zeros((T, 4, 4), np.float32)
    q = rng.standard_normal(4)
    t = rng.standard_normal(3) * 0.1
    for f in range(T):
        q = q / np.linalg.norm(q) + spread * rng.standard_normal(4)
        t = t + 0.05 * rng.standard_normal(3)
        out[f, :3, :3] = O.quaternion_to_matrix((q / np.linalg.norm(q))[None])[0]
        out[f, :3, 3] = t
        out[f, 3] = (500, 500, 256, 256)
    return out


def main():
    install_trimesh()
    _, nerf, _, _ = _ref_import.import_reference()
    import importlib
    lu = importlib.import_module("nnutils.loss_utils")
    proxy = TorchProxy()
    lu.torch = proxy
    rng = np.random.default_rng(36)
    out = {}

    # ---- shape_init_loss
    torch.manual_seed(36)
    net = nerf.NeRF(D=5, W=64, in_channels_xyz=63)
    emb = nerf.Embedding(3, 10)
    weights = {k: v.detach().clone() for k, v in net.state_dict().items()}
    verts = (rng.uniform(-1, 1, (V, 3)) * np.asarray([1.0, 0.6, 0.35]) * 0.1).astype(np.float32)
    out["shape/pts"], out["shape/bound_factor"] = verts, np.float64(BOUND_FACTOR)
    for k, v in weights.items():
        out[f"shape/w/{k}"] = v.numpy()
    for mode, ellips in (("ellips", True), ("sphere", False)):
        for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
            m = nerf.NeRF(D=5, W=64, in_channels_xyz=63).to(dt)
            m.load_state_dict({k: v.to(dt) for k, v in weights.items()})
            seen = {}

            def hook(_m, inp, o):
                seen["y"] = o
                o.retain_grad()
            h1 = m.register_forward_hook(hook)
            h2 = emb.register_forward_pre_hook(lambda _m, inp: seen.__setitem__("pts_samp", inp[0].detach().clone()))
            torch.manual_seed(360 + int(ellips))                         # the same draw for both precisions
            loss = lu.shape_init_loss(torch.from_numpy(verts).to(dt), torch.zeros(1, 3, dtype=torch.int64), m, emb,
                                      bound_factor=BOUND_FACTOR, use_ellips=ellips)
            loss.backward()
            h1.remove()
            h2.remove()
            u = proxy.u.reshape(NSAMPLE, 3).numpy()
            if f"shape/{mode}/u" in out:
                assert np.array_equal(out[f"shape/{mode}/u"], u)
            out[f"shape/{mode}/u"] = u
            pre = f"shape/{mode}/{prec}/"
            out[pre + "pts_samp"] = seen["pts_samp"].reshape(NSAMPLE, 3).numpy()
            out[pre + "y"] = seen["y"].detach().reshape(-1).numpy()
            out[pre + "dy"] = seen["y"].grad.reshape(-1).numpy()
            out[pre + "loss"] = loss.detach().numpy()
            if ellips:
                for k, p in m.named_parameters():
                    if p.grad is not None:
                        out[pre + "d/" + k] = p.grad.numpy()

    # ---- rtk_loss: a noisy prediction of a table; frame 3 equals its target (clamp at the top), frame 5 is half a turn away
    raw = poses(rng, RTK_T, 0.2)
    pred = poses(rng, RTK_T, 0.2)
    pred[3, :3, :3] = raw[3, :3, :3]
    pred[5, :3, :3] = (raw[5, :3, :3].astype(np.float64) @ np.diag([1., -1., -1.])).astype(np.float32)
    out["rtk/pred"], out["rtk/raw"] = pred, raw
    for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
        for which in ("total", "rot"):
            p = torch.from_numpy(pred).to(dt).requires_grad_(True)
            aux = {}
            total = lu.rtk_loss(p, torch.from_numpy(raw).to(dt), aux)
            (total if which == "total" else aux["rot_loss"]).backward()
            out[f"rtk/{prec}/d_{which}"] = p.grad.numpy()
        out[f"rtk/{prec}/total"] = total.detach().numpy()
        out[f"rtk/{prec}/rot_loss"] = aux["rot_loss"].detach().numpy()
        out[f"rtk/{prec}/trn_loss"] = aux["trn_loss"].detach().numpy()

    # ---- compute_root_sm_loss: videos of 1, 2, 3 and 34 frames; frames 10 and 11 are the same pose (zero difference)
    sm = poses(rng, SM_OFFSET[-1], 0.05)
    sm[11] = sm[10]
    out["sm/rtk"], out["sm/data_offset"] = sm, np.asarray(SM_OFFSET, np.int64)
    for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
        p = torch.from_numpy(sm).to(dt).requires_grad_(True)
        loss = lu.compute_root_sm_loss(p, list(SM_OFFSET))
        loss.backward()
        assert torch.isfinite(p.grad).all()
        out[f"sm/{prec}/loss"], out[f"sm/{prec}/d"] = loss.detach().numpy(), p.grad.numpy()

    path = os.path.join(HERE, "g36_warmup.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
