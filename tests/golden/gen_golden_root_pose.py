"""Generate tests/golden/g32_root_pose.npz by running the reference's own root-pose modules on the CPU (development container
only, like gen_golden_lossasm.py): RTHead with both use_quat values, RTExplicit and RTExpMLP with both delta values
(nnutils/nerf.py:307-344, 382-470), and refine_rt, create_base_se3, prepare_ray_cams over K2mat / K2inv / Kmatinv
(nnutils/geom_utils.py:596-652) -- outputs and the gradients of sum(w * out) for a recorded random w, in fp32 and in float64,
and per output d_ref = max |fp32 - float64| of the reference itself -- for the modules above, and (the d_ref alone) for the
composed tail at every shape the GPU tests run and for the chain into raycast (geom_utils.py:746-794).  Inputs and outputs only: the network weights come from
moda_amd.synth by seed (tests/rootpose_cases.py) and are not stored.

pytorch3d is absent here and unpinned; tests/golden/_ref_import.py stubs its quaternion helpers, and this generator adds
so3_exponential_map to the stub as the published formula: theta = sqrt(clamp(sum(w * w), min=1e-4)),
R = sin(theta) / theta hat(w) + (1 - cos(theta)) / theta^2 hat(w)^2 + I.

FrameCode computes its time coordinate in fp32 whatever the module's dtype (a .double() RTExpMLP raises inside basis_mlp), so
the float64 recording of RTExpMLP starts from the fp32 frame code cast to double.

nnutils/moda.py cannot be imported here (absl flags, mcubes): the three static methods recorded from it -- refine_rt,
create_base_se3, prepare_ray_cams -- are compiled on their own from its syntax tree; compute_rts and convert_root_pose read
their inputs off the model object, so they are restated in tests/rootpose_numpy.py and not recorded.

    python tests/golden/gen_golden_root_pose.py
"""
import ast
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import  # noqa: E402
import rootpose_cases as C  # noqa: E402


def so3_exponential_map(log_rot, eps=1e-4):
    nrm = (log_rot * log_rot).sum(1)
    theta = torch.clamp(nrm, min=eps).sqrt()
    f1 = theta.sin() / theta
    f2 = (1 - theta.cos()) / (theta * theta)
    K = log_rot.new_zeros((log_rot.shape[0], 3, 3))
    x, y, z = log_rot.unbind(1)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -z, y, z, -x, -y, x
    return f1[:, None, None] * K + f2[:, None, None] * torch.bmm(K, K) + torch.eye(3, dtype=log_rot.dtype)[None]


def moda_static_methods(geom):
    """refine_rt, create_base_se3, prepare_ray_cams of nnutils/moda.py, compiled from its syntax tree without importing it."""
    tree = ast.parse(open(os.path.join(_ref_import.REF, "nnutils", "moda.py")).read())
    want, ns = ("refine_rt", "create_base_se3", "prepare_ray_cams"), {"torch": torch, "K2mat": geom.K2mat, "K2inv": geom.K2inv,
                                                                      "Kmatinv": geom.Kmatinv}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in want:
            node.decorator_list = []
            exec(compile(ast.Module([node], []), "moda.py", "exec"), ns)
    return [ns[k] for k in want]


class Const(nn.Module):
    def __init__(self, value):
        super().__init__()
        self.value = value

    def forward(self, _):
        return self.value


def T(a, dt):
    return torch.from_numpy(np.asarray(a)).to(dt)


def record(out, name, run):
    """run(dtype) -> (output, {grad name: tensor}); stores both precisions and the reference's own fp32 error."""
    res = {}
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        o, grads = run(dt)
        res[tag] = {"out": o.detach().numpy(), **{(k[1:] if k[0] == "=" else "d_" + k): v.detach().numpy() for k, v in grads.items()}}
    for k in res["32"]:
        out[f"{name}_{k}_32"], out[f"{name}_{k}_64"] = res["32"][k], res["64"][k]
        out[f"{name}_dref_{k}"] = np.asarray(np.abs(res["32"][k].astype(np.float64) - res["64"][k]).max())


def record_tails(out, nerf, refine_rt):
    """d_ref of the composed tail (RTExpMLP.forward over given base and delta rows, then refine_rt) at every shape, pair of
    rotation forms and refine_rt form that tests/test_gpu_rootpose.py runs: only the three scalars per case are stored.  The
    delta rows reach RTHead's own tail through a NeRF.forward that returns its input."""
    mlp_forward = nerf.NeRF.forward
    nerf.NeRF.forward = lambda self, x, *a, **k: x
    try:
        for n in C.TAIL_N:
            for cols, dcols in C.TAIL_COLS:
                c = C.tail_case(n, cols, dcols)
                for form, obj_scale in C.TAIL_RAW:
                    res = {}
                    for dt in (torch.float32, torch.float64):
                        m = nerf.RTExpMLP(c["T"], C.NUM_FREQS, C.CODE, np.asarray([0, c["T"]]), delta=cols == 6)
                        m.base_rt.se3.data = torch.from_numpy(c["se3"])
                        m = m.to(dt)
                        rows = T(c["delta"], dt).requires_grad_(True)
                        head = nerf.RTHead(use_quat=dcols == 7, D=1, W=8, in_channels_xyz=dcols, in_channels_dir=0,
                                           out_channels=dcols, raw_feat=True)
                        m.delta_rt = nn.Sequential(Const(rows), head)
                        ids = torch.from_numpy(c["ids"])
                        root = m(ids)
                        if form == "base":
                            rt = torch.zeros(n, 3, 4, dtype=dt)
                            rt[:, 0, 0] = rt[:, 1, 1] = rt[:, 2, 2] = 1
                            rt[:, 2, 3] = float(np.float32(0.3))
                        else:
                            rt = T(c["raw"][:n] if form == "rows" else c["raw"][:c["T"]][c["ids"]], dt).clone()
                            rt[:, :3, 3] = rt[:, :3, 3] / obj_scale
                        o = refine_rt(rt, root)
                        (T(c["g"][:, :3], dt) * o).sum().backward()
                        res[dt] = (o.detach().numpy(), m.base_rt.se3.grad.numpy(), rows.grad.numpy())
                    for k, name in enumerate(("rtk", "d_se3", "d_delta")):
                        out[C.tail_key(n, cols, dcols, form, name)] = np.asarray(
                            np.abs(res[torch.float32][k].astype(np.float64) - res[torch.float64][k]).max())
    finally:
        nerf.NeRF.forward = mlp_forward


def record_chain(out, nerf, geom, refine_rt, prepare_ray_cams, kaug):
    """d_ref of RTExpMLP -> refine_rt on create_base_se3 -> K row -> prepare_ray_cams -> raycast -> sum(w_d rays_d + w_o rays_o)."""
    c = C.chain_case()
    off = np.asarray(C.DATA_OFFSET)
    sd = {k: torch.from_numpy(v) for k, v in C.expmlp_state(False).items()}
    m32 = nerf.RTExpMLP(C.T, C.NUM_FREQS, C.CODE, off)
    m32.load_state_dict(sd, strict=True)
    fid = torch.from_numpy(c["fid"])
    code32 = m32.root_code(fid).detach()

    def run(dt):
        if dt == torch.float64:
            torch.set_default_dtype(torch.float64)
        try:
            m = nerf.RTExpMLP(C.T, C.NUM_FREQS, C.CODE, off)
            m.load_state_dict(sd, strict=True)
            if dt == torch.float64:
                m = m.double()
                m.delta_rt = nn.Sequential(Const(code32.double()), m.mlp_rt)
            ks = T(c["ks"], dt).requires_grad_(True)
            rt = torch.zeros(4, 3, 4, dtype=dt)
            rt[:, 0, 0] = rt[:, 1, 1] = rt[:, 2, 2] = 1
            rt[:, 2, 3] = float(np.float32(0.3))
            rtk = torch.cat([refine_rt(rt, m(fid)), ks[torch.from_numpy(c["did"])][:, None]], 1)
            rays = geom.raycast(T(c["xys"], dt), *prepare_ray_cams(rtk, T(kaug, dt)), None)
            ((T(c["wd"], dt) * rays["rays_d"]).sum() + (T(c["wo"], dt) * rays["rays_o"]).sum()).backward()
        finally:
            torch.set_default_dtype(torch.float32)
        return rays["rays_d"], {"=rays_o": rays["rays_o"], "se3": m.base_rt.se3.grad, "rgb": m.mlp_rt.rgb[0].weight.grad, "ks": ks.grad}
    record(out, "chain", run)


def main():
    _ref_import.install_stubs()
    sys.modules["pytorch3d.transforms"].so3_exponential_map = so3_exponential_map
    _, nerf, geom, _ = _ref_import.import_reference()
    refine_rt, create_base_se3, prepare_ray_cams = moda_static_methods(geom)
    out = {}

    # RTHead, both forms
    x = C.synth.normal(C.SEED, "g32/x", (8, C.CODE))
    out["x"] = x
    for tag, use_quat, n_out in (("rthead_q", True, 7), ("rthead_w", False, 6)):
        w = C.weight(tag, (8, 1, 12))
        out[tag + "_w"] = w

        def run(dt, use_quat=use_quat, n_out=n_out, tag=tag, w=w):
            m = nerf.RTHead(use_quat=use_quat, out_channels=n_out, raw_feat=True, **C.HEAD_KW)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in C.head_params(tag, n_out).items()})
            m = m.to(dt)
            xi = T(x, dt).requires_grad_(True)
            o = m(xi)
            (T(w, dt) * o).sum().backward()
            return o, {"x": xi.grad, "rgb": m.rgb[0].weight.grad}
        record(out, tag, run)

    # RTExplicit on the edge-case rows, both forms
    for tag, delta in (("exp_q", False), ("exp_w", True)):
        w = C.weight(tag, (len(C.EDGE_IDS), 1, 12))
        out[tag + "_w"] = w

        def run(dt, delta=delta, w=w):
            m = nerf.RTExplicit(8, delta=delta, rand=False)
            m.se3.data = torch.from_numpy(C.se3_table(delta, 8))
            m = m.to(dt)
            o = m(torch.from_numpy(C.EDGE_IDS))
            (T(w, dt) * o).sum().backward()
            return o, {"se3": m.se3.grad}
        record(out, tag, run)

    # RTExpMLP, both forms
    off = np.asarray(C.DATA_OFFSET)
    for tag, delta in (("expmlp_q", False), ("expmlp_w", True)):
        w = C.weight(tag, (len(C.IDS), 1, 12))
        out[tag + "_w"] = w
        m32 = nerf.RTExpMLP(C.T, C.NUM_FREQS, C.CODE, off, delta=delta)
        out["expmlp_keys"] = np.asarray(list(m32.state_dict().keys()))
        m32.load_state_dict({k: torch.from_numpy(v) for k, v in C.expmlp_state(delta).items()}, strict=True)
        code32 = m32.root_code(torch.from_numpy(C.IDS)).detach()
        out[tag + "_code_32"] = code32.numpy()

        def run(dt, delta=delta, w=w, code32=code32):
            m = nerf.RTExpMLP(C.T, C.NUM_FREQS, C.CODE, off, delta=delta)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in C.expmlp_state(delta).items()}, strict=True)
            code = None
            if dt == torch.float64:
                m = m.double()
                code = code32.double().requires_grad_(True)
                m.delta_rt = nn.Sequential(Const(code), m.mlp_rt)
            o = m(torch.from_numpy(C.IDS))
            (T(w, dt) * o).sum().backward()
            return o, {"se3": m.base_rt.se3.grad, "rgb": m.mlp_rt.rgb[0].weight.grad}
        record(out, tag, run)

    # refine_rt, create_base_se3, prepare_ray_cams and the intrinsics helpers
    n = 8
    rt_raw = np.zeros((n, 4, 4), np.float32)
    rt_raw[:, :3, :3] = out["exp_q_out_64"][:n, 0, :9].reshape(n, 3, 3)
    rt_raw[:, :3, 3] = C.synth.normal(C.SEED, "g32/raw_t", (n, 3))
    rt_raw[:, 3] = np.abs(C.synth.normal(C.SEED, "g32/raw_k", (n, 4))) * np.float32(100) + np.float32([300, 500, 200, 250])
    kaug = (np.abs(C.synth.normal(C.SEED, "g32/kaug", (n, 4))) + np.float32([0.5, 0.8, 0.1, 0.2])).astype(np.float32)
    root = out["expmlp_q_out_32"]
    out.update({"refine_rt_raw": rt_raw, "refine_root": root, "kaug": kaug})
    assert torch.equal(create_base_se3(3, "cpu"), T(np.tile(np.asarray([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.3]], np.float32), (3, 1, 1)),
                                                   torch.float32))
    out["base_se3"] = create_base_se3(3, "cpu").numpy()
    wr, wR, wT, wK = (C.weight(k, s) for k, s in (("refine", (n, 4, 4)), ("cams_R", (n, 3, 3)), ("cams_T", (n, 3)), ("cams_K", (n, 3, 3))))
    out.update({"refine_w": wr, "cams_wR": wR, "cams_wT": wT, "cams_wK": wK})

    def run_refine(dt):
        r = T(root, dt).requires_grad_(True)
        o = refine_rt(T(rt_raw, dt), r)
        (T(wr, dt) * o).sum().backward()
        return o, {"root": r.grad}
    record(out, "refine", run_refine)

    def run_cams(dt):
        # K2mat / K2inv allocate fp32 whatever their input: the float64 run casts their results as the reference's lines do not
        if dt == torch.float64:
            torch.set_default_dtype(torch.float64)
        try:
            r = T(rt_raw, dt).requires_grad_(True)
            Rm, Tm, Ki = prepare_ray_cams(r, T(kaug, dt))
            ((T(wR, dt) * Rm).sum() + (T(wT, dt) * Tm).sum() + (T(wK, dt) * Ki).sum()).backward()
            extra = {"=Tmat": Tm, "=Kinv": Ki, "=K2inv": geom.K2inv(T(kaug, dt)), "=Kmatinv": geom.Kmatinv(geom.K2mat(T(rt_raw[:, 3], dt)))}
        finally:
            torch.set_default_dtype(torch.float32)
        return Rm, {"rtk": r.grad, **extra}
    record(out, "cams", run_cams)

    record_tails(out, nerf, refine_rt)
    record_chain(out, nerf, geom, refine_rt, prepare_ray_cams, kaug[:4])

    path = os.path.join(HERE, "g32_root_pose.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        if "_dref_" in k:
            print(f"  {k:28s} {float(out[k]):.3e}")


if __name__ == "__main__":
    main()
