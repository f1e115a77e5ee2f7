"""Inputs shared by tests/golden/gen_golden_root_pose.py, tests/test_rootpose_oracle.py and tests/test_gpu_rootpose.py: network
weights from moda_amd.synth by seed (never stored), the edge-case pose rows, and the comparison rule of the GPU tests."""
import numpy as np

from moda_amd import synth

SEED = 32
T, DATA_OFFSET, NUM_FREQS, CODE = 65, (0, 40, 65), 6, 128
IDS = np.asarray([0, 3, 39, 40, 41, 64, 3, 3], np.int64)           # both videos, their ends, one frame three times
HEAD_KW = dict(D=8, W=256, in_channels_xyz=CODE, in_channels_dir=0)


def head_params(name, out_channels):
    """State dict (numpy) of an RTHead-shaped NeRF."""
    return synth.nerf_params(SEED, "g32/" + name, out_channels=out_channels, **HEAD_KW)


def rotvec_rows():
    """Rotation vectors at the places so3_exp changes behaviour: zero, |w|^2 either side of the 1e-4 clamp, |w| near pi."""
    d = synth.normal(SEED, "g32/rotvec_dirs", (8, 3)).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    norms = np.asarray([0.0, np.sqrt(0.9e-4), np.sqrt(1.1e-4), np.pi - 1e-3, 0.3, 1.2, 2.5, 0.05])
    return (d * norms[:, None]).astype(np.float32)


def quat_rows():
    """Unnormalised quaternions: norms 1e-3 and 1e3, a negative real part, and ordinary ones."""
    q = synth.normal(SEED, "g32/quats", (8, 4)).astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[2, 0] = -abs(q[2, 0]) - 0.5
    scale = np.asarray([1e-3, 1e3, 1.0, 0.7, 1.0, 2.0, 1.0, 1.3])
    return (q * scale[:, None]).astype(np.float32)


def se3_table(delta, rows=T):
    """(rows, 6 | 7) pose table whose first eight rows are the edge cases."""
    edge = rotvec_rows() if delta else quat_rows()
    rot = synth.normal(SEED, f"g32/se3_rot{int(delta)}", (rows, edge.shape[1])) * np.float32(0.5 if delta else 1.0)
    rot[:min(8, rows)] = edge[:rows]
    trans = synth.normal(SEED, f"g32/se3_t{int(delta)}", (rows, 3))
    return np.concatenate([trans, rot], -1).astype(np.float32)


EDGE_IDS = np.asarray([0, 1, 2, 3, 4, 5, 6, 7, 3, 1], np.int64)


def expmlp_state(delta, rows=T, data_offset=DATA_OFFSET):
    """The reference's 55 state-dict entries of an RTExpMLP."""
    n_in = (len(data_offset) - 1) * (1 + 2 * NUM_FREQS)
    w, b = synth.linear_init(SEED, "g32/root_code", CODE, n_in)
    mlp = head_params("mlp_rt", 6)
    sd = {"root_code.basis_mlp.weight": w, "root_code.basis_mlp.bias": b, "base_rt.se3": se3_table(delta, rows)}
    sd.update({"mlp_rt." + k: v for k, v in mlp.items()})
    sd.update({"delta_rt.0.basis_mlp.weight": w, "delta_rt.0.basis_mlp.bias": b})
    sd.update({"delta_rt.1." + k: v for k, v in mlp.items()})
    return sd


TAIL_N = (1, 63, 64, 65, 257)
TAIL_COLS = ((7, 6), (6, 7), (6, 6), (7, 7))
TAIL_T = {1: 1, 63: 3, 64: 65, 65: 65, 257: 65}
TAIL_RAW = (("base", 1.0), ("rows", 1.7), ("by_id", 0.6))          # refine_rt form, obj_scale


def tail_case(n, cols, dcols):
    """Inputs of one tail call at n rows: base table (T, cols), delta rows (n, dcols), ids, intrinsics, cotangent, raw poses.
    Quaternion norms lie in [0.7, 1.5]: a row's gradient grows as 1 / |q|, which the edge rows (|q| = 1e-3, 1e3) cover."""
    rng = np.random.default_rng(100 * n + cols * 10 + dcols)
    Tn = TAIL_T[n]
    se3 = np.concatenate([rng.normal(size=(Tn, 3)), rng.normal(size=(Tn, cols - 3)) * (1.0 if cols == 7 else 0.6)], -1).astype(np.float32)
    delta = np.concatenate([rng.normal(size=(n, 3)), rng.normal(size=(n, dcols - 3)) * (1.0 if dcols == 7 else 0.2)], -1).astype(np.float32)
    for rows_, c_ in ((se3, cols), (delta, dcols)):
        if c_ == 7:
            q = rows_[:, 3:].astype(np.float64)
            rows_[:, 3:] = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.7, 1.5, size=(len(q), 1))).astype(np.float32)
    ids = rng.integers(0, Tn, size=n)
    ks = (np.abs(rng.normal(size=(2, 4))) * 50 + [300, 500, 200, 250]).astype(np.float32)
    dataid = (ids >= 40).astype(np.int64) if Tn == 65 else np.zeros(n, np.int64)
    g = rng.normal(size=(n, 4, 4)).astype(np.float32)
    w = rng.normal(size=(max(n, Tn), 3))
    th = np.linalg.norm(w, axis=1)[:, None, None]
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    raw = np.zeros((len(w), 3, 4), np.float32)
    raw[:, :, :3] = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    raw[:, :, 3] = rng.normal(size=(len(raw), 3))
    return dict(T=Tn, se3=se3, delta=delta, ids=ids, ks=ks, dataid=dataid, g=g, raw=raw)


def tail_key(n, cols, dcols, form, out):
    return f"tail_{n}_{cols}{dcols}_{form}_dref_{out}"


def chain_case():
    """convert_root_pose -> prepare_ray_cams -> raycast, 4 frames x 8 pixels."""
    return dict(fid=np.asarray([3, 39, 40, 3]), did=np.asarray([0, 0, 1, 0]),
                ks=np.asarray([[300., 500., 200., 250.], [310., 505., 215., 260.]], np.float32),
                xys=synth.uniform(SEED, "g32/xys", (4, 8, 2)) * np.float32(512),
                wd=weight("chain_d", (4, 8, 3)), wo=weight("chain_o", (4, 8, 3)))


def weight(name, shape):
    """The random cotangent of sum(w * out)."""
    return synth.normal(SEED, "g32/w/" + name, shape)


def allowance(ref64, d_ref):
    """What a fp32 result may differ from the float64 restatement by: 4 x the reference's own fp32 error for that output, and
    not less than 4 ulp of the output's largest magnitude."""
    top = float(np.abs(np.asarray(ref64)).max())
    return max(4.0 * float(d_ref), 4.0 * float(np.spacing(np.float32(top))))
