"""Float64 numpy restatement of moda_amd/animate.py: the frame-independent skinning weights, the all-frames forward warp
(geom_utils.py:1029-1073 with FrameCode, nerf.py:346-380, DQ_RTHead, :239-279, correct_bones / correct_rest_pose,
geom_utils.py:933-972), get_vertex_colors' input rows (utils/io.py:559-582), save_bones (:51-78) and the skin colours
(train_utils.py:582-590).  Built on the repository's CPU oracle (oracle/moda_oracle.py, pinned to the reference by
test_oracle_vs_golden.py) and on warp_numpy's point transform; inputs are widened, never re-rounded.  The one fp32 step is
FrameCode's time coordinate, which the reference computes in fp32 whatever the module's dtype.  Nothing here imports the package's
compute path."""
import colorsys

import numpy as np

import warp_numpy as WN
from oracle import moda_oracle as orc


def f64(d):
    if isinstance(d, dict):
        return {k: f64(v) for k, v in d.items()}
    return np.asarray(d, np.float64)


def mock_params(B=25, seed=13, tag="g13"):
    """The fp32 parameters of the mock model of tests/golden/gen_golden.py g13 (B = 25: the very model g13_grid.npz was written
    from; other B: the same recipe), as the dict the functions below take.  The GPU tests load the same arrays into the package."""
    from moda_amd import synth
    C = 128
    head = synth.nerf_params(seed, f"{tag}/head", D=8, W=256, in_channels_xyz=C, in_channels_dir=0, out_channels=7 * B)
    head["rgb.0.weight"] = head["rgb.0.weight"] * np.float32(0.05)
    head["rgb.0.bias"] = np.tile(np.asarray([0, 0, 0, 1, 0, 0, 0], np.float32), B) \
        + np.float32(0.1) * synth.normal(seed, f"{tag}/head/b", (7 * B,))
    fw, fb = synth.linear_init(seed, f"{tag}/pose", C, 2 * (1 + 2 * 6))
    mp = synth.make_models(seed, B=B, with_skin=True, with_vis=True, perturb_bones=True, with_dis=True)
    return dict(bones=mp["bones_rst"], skin_aux=mp["skin_aux"], nerf_skin=mp["nerf_skin"], nerf_dis=mp["nerf_dis"],
                rest_pose_code=mp["rest_pose_code"], head=head, pose_w=fw[:, :13], pose_b=fb, num_freq=6, vid_offset=[0, 50],
                coarse=mp["coarse"], nerf_vis=mp["nerf_vis"], alpha=10.0)


# ---- per-frame codes and transforms -------------------------------------------------------------------------------------------
def frame_code(fids, num_freq, vid_offset, weight, bias, scale=1.0):
    """FrameCode.forward: fids (n,) -> (n, C) = Linear(one-hot(video) (x) Fourier(t))."""
    fids = np.asarray(fids).reshape(-1)
    vo = np.asarray(vid_offset)
    nv = len(vo) - 1
    max_ts = np.float32((vo[1:] - vo[:-1]).max())
    tid = np.zeros(len(fids), np.float32)
    vid = np.zeros(len(fids), np.int64)
    for i in range(nv):
        a = (fids >= vo[i]) & (fids < vo[i + 1])
        vid[a] = i
        d = np.float32(vo[i + 1] - vo[i])
        tid[a] = (fids[a].astype(np.float32) - np.float32(vo[i]) - d / np.float32(2)) / max_ts * np.float32(2)    # geom_utils.py:1776
    coeff = orc.embedding((tid * np.float32(scale)).astype(np.float64)[:, None], num_freq, num_freq)             # (n, 1 + 2 F)
    wide = np.zeros((len(fids), coeff.shape[1], nv))
    wide[np.arange(len(fids)), :, vid] = coeff
    return wide.reshape(len(fids), -1) @ f64(weight).T + f64(bias)


def dq_rthead(code, head):
    """DQ_RTHead.forward: code (n, C) -> (n, 8 B) unit dual quaternions [r | 0.5 (0, t) (x) r], t = 0.1 out[:3]."""
    head = f64(head)
    D, W, in_xyz, in_dir, _ = orc._mlp_dims(head)
    y = orc.nerf_forward(head, f64(code), D=D, W=W, in_channels_xyz=in_xyz, in_channels_dir=in_dir, raw_feat=True)
    rts = y.reshape(-1, 7)
    rq = rts[:, 3:7] / np.maximum(np.sqrt((rts[:, 3:7] ** 2).sum(-1, keepdims=True)), 1e-12)
    tq = np.concatenate([np.zeros_like(rts[:, :1]), rts[:, :3] * 0.1], -1)
    return np.concatenate([rq, 0.5 * orc.quaternion_raw_multiply(tq, rq)], -1).reshape(len(y), -1)


def rest_pose(m):
    """correct_bones: -> (bones_rst (B, 10), bone_rts_rst (1, 8 B))."""
    rst = dq_rthead(f64(m["rest_pose_code"])[:1], m["head"])
    return orc.bone_transform(f64(m["bones"]), rst)[0], rst


def correct_rest_pose(rts_fw, rts_rst, B):
    fw = f64(rts_fw).reshape(-1, B, 8)
    inv = np.ascontiguousarray(np.broadcast_to(orc.dq_inverse(f64(rts_rst).reshape(1, B, 8)), fw.shape))
    return orc.dq_mul(inv, np.ascontiguousarray(fw))


def _scene(m, bones_rst, nerf_skin):
    return orc.Scene(None, bones_rst=bones_rst, skin_aux=f64(m["skin_aux"]), nerf_skin=f64(m["nerf_skin"]) if nerf_skin else None,
                     rest_pose_code=f64(m["rest_pose_code"]), nerf_dis=f64(m["nerf_dis"]) if "nerf_dis" in m else None,
                     alpha_xyz=m.get("alpha", 10.0))


def skin_weights(m, vertices, nerf_skin=True):
    """-> (V, B): gauss_mlp_skinning at the rest vertices with rest_pose_code and the corrected rest bones."""
    bones_rst, _ = rest_pose(m)
    v = f64(vertices)[None]
    return orc.gauss_mlp_skinning(_scene(m, bones_rst, nerf_skin), v, bones_rst, f64(m["rest_pose_code"])[:1])[0]


def displaced_vertices(m, vertices):
    v = f64(vertices)
    return v + orc.residual_deformation(_scene(m, None, False), v[None], f64(m["rest_pose_code"])[:1])[0]


def dqs_frames(dq, skin, pts):
    """dq (F, B, 8), skin (V, B), pts (V, 3) -> (F, V, 3), dqs_blend_skinning_chunk; a vanishing real part gives NaN (0 / 0) as
    the arithmetic does, without the oracle's assertion."""
    bl = np.einsum("vb,fbk->fvk", f64(skin), f64(dq))
    with np.errstate(divide="ignore", invalid="ignore"):
        c = bl / np.sqrt((bl[..., :4] ** 2).sum(-1, keepdims=True))
        return WN._transform(c, np.broadcast_to(f64(pts)[None], bl.shape[:2] + (3,)))


def frame_transforms(m, embedids):
    """-> (rts (F, B, 8) relative to the rest pose, bones (F, B, 10) posed, bones_rst)."""
    B = len(m["bones"])
    bones_rst, rst = rest_pose(m)
    code = frame_code(embedids, m["num_freq"], m["vid_offset"], m["pose_w"], m["pose_b"])
    rts = correct_rest_pose(dq_rthead(code, m["head"]), rst, B)
    return rts, orc.bone_transform(bones_rst, rts.reshape(len(rts), -1)), bones_rst


def warp_fw_frames(m, vertices, embedids, nerf_skin=True, nerf_dis=False):
    """-> (verts (F, V, 3), bones (F, B, 10))."""
    rts, bones, _ = frame_transforms(m, embedids)
    skin = skin_weights(m, vertices, nerf_skin)
    p = displaced_vertices(m, vertices) if nerf_dis else f64(vertices)
    return dqs_frames(rts, skin, p), bones


# ---- vertex colours ---------------------------------------------------------------------------------------------------------------
def color_rows(verts_frames, rtks, env_rows, n_freq=4, alpha=4.0, n_vertices=None):
    """The `dir_src` rows of get_vertex_colors: (F V, 3 (1 + 2 n_freq) + Ce) = [Embedding(normalize(v - cam centre)) | env row];
    verts_frames None: the fixed direction (0, 0, -1) for n_vertices vertices."""
    env = f64(env_rows)
    F = len(env)
    if verts_frames is None:
        d = np.zeros((F, n_vertices, 3))
        d[..., 2] = -1
    else:
        v, k = f64(verts_frames), f64(rtks)
        cam = -np.einsum("fji,fj->fi", k[:, :3, :3], k[:, :3, 3])                     # -R^T t
        d = v - cam[:, None]
        d = d / np.maximum(np.sqrt((d * d).sum(-1, keepdims=True)), 1e-12)
    V = d.shape[1]
    emb = orc.embedding(d.reshape(-1, 3), n_freq, alpha)
    return np.concatenate([emb, np.repeat(env, V, 0)], -1)


def vertex_colors_frames(coarse, rest_vertices, verts_frames, rtks, env_rows, n_freq_xyz=10, alpha_xyz=10.0, n_freq_dir=4,
                         alpha_dir=4.0):
    """coarse: x (N, 63 + 27 + Ce) float64 -> (N, >= 3), the network's forward (the caller's; the GPU test passes the package's
    own layer-by-layer nerf_coarse).  -> (F, V, 3) in [0, 1]."""
    rest = f64(rest_vertices)
    rows = color_rows(verts_frames, rtks, env_rows, n_freq_dir, alpha_dir, n_vertices=len(rest))
    F = len(rows) // len(rest)
    x = np.concatenate([np.tile(orc.embedding(rest, n_freq_xyz, alpha_xyz), (F, 1)), rows], -1)
    return np.clip(f64(coarse(x))[:, :3], 0, 1).reshape(F, len(rest), 3)


# ---- bones as ellipsoids, skin colours ------------------------------------------------------------------------------------------
def quat_to_matrix(q):
    """Unit quaternion (.., 4), real first -> (.., 3, 3), written out."""
    r, i, j, k = (q[..., n] for n in range(4))
    return np.stack([1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r),
                     2 * (i * j + k * r), 1 - 2 * (i * i + k * k), 2 * (j * k - i * r),
                     2 * (i * k - j * r), 2 * (j * k + i * r), 1 - 2 * (i * i + j * j)], -1).reshape(q.shape[:-1] + (3, 3))


def bone_ellipsoids(bones, template):
    """bones (F, B, 10), template (Nv, 3) -> (F, B Nv, 3): centre + R(q / |q|) (t / exp(scale))."""
    b, t = f64(bones), f64(template)
    q = b[..., 3:7] / np.sqrt((b[..., 3:7] ** 2).sum(-1, keepdims=True))
    s = t[None, None] / np.exp(b[..., None, 7:10])                                # (F, B, Nv, 3)
    out = b[..., None, :3] + np.einsum("fbij,fbnj->fbni", quat_to_matrix(q), s)
    return out.reshape(b.shape[0], -1, 3)


def skin_colors(skin, palette):
    return (f64(palette)[None] * f64(skin)[..., None]).sum(1)


def default_palette(n):
    """The package's stated rule: hue frac(i * golden-ratio conjugate), saturation 0.55 + 0.15 (i mod 3), value 0.95."""
    return np.asarray([[int(round(255 * c)) for c in colorsys.hsv_to_rgb((i * 0.618033988749895) % 1.0, 0.55 + 0.15 * (i % 3), 0.95)]
                       for i in range(n)], np.uint8).reshape(n, 3)
