"""Mesh sequence export, device-resident: what v2s_trainer.eval(dynamic_mesh=True) (nnutils/train_utils.py:455-624) produces per
frame and extract.py:24-53 writes -- the rest mesh warped to every frame, the frame's bones as ellipsoids, the camera, a
skin-coloured rest mesh, view-dependent vertex colours -- for ALL frames of a sequence at once.

In the forward direction the skinning weights do not depend on the frame: gauss_mlp_skinning runs on the rest vertices with
rest_pose_code and the corrected rest bones (geom_utils.py:1046-1059), and only the B dual quaternions change.  mesh_queries.warp_fw
re-evaluates them on every call; here `skin_weights` (and `displaced_vertices`) run once, and moda_dqs_frames
(csrc/animate_kernels.hip) applies every frame's transforms in one launch.  The host reads nothing back in skin_weights,
warp_fw_frames, vertex_colors_frames, bone_ellipsoids, skin_colors and export_sequence; MeshSequence.save is the one place the
device is copied out, once per array (MeshSequence.frame(i) hands out device views; a TriMesh copies on first host access).

Deviations from the reference, all deliberate:
  * The ellipsoid template is this module's own UV sphere (`uv_sphere`: poles plus RINGS - 1 rings of SEGMENTS vertices, 242
    vertices and 480 faces at the default 16 x 16), not trimesh.creation.uv_sphere(count=[16, 16]): trimesh is absent and unpinned,
    and the vertex and face counts are NOT claimed equal to it.  Radius len_max / 20 as in the reference.
  * The default palette is `default_palette`, a fixed hue walk, not the reference's label_colormap table; a caller who wants those
    colours passes them in.  The reference tiles its table fourfold (train_utils.py:585); a palette shorter than B is refused.
  * vertex_colors_frames takes `env_ids` explicitly: the reference passes the index WITHIN THE BATCH as the frame of the
    environment code (frame_idx=idx, train_utils.py:544-545), not the frame id.  The choice is the caller's.
  * Colours become 8-bit by truncation of value * 255, which is what assigning a float array to trimesh's uint8 colours does.
  * OBJ files carry `v x y z r g b` with colours as 0..1 floats and 1-based `f` lines, nothing else (no normals, no header).
  * lbs and the flow warps are refused with NotImplementedError, as everywhere in this package.  Inference only.
Out of scope: the rendered images, flow and videos of eval() / extract.py, draw_cams' camera mesh."""
import colorsys
import os

import numpy as np
import torch

from . import _lib as L
from . import abi
from .feeders import correct_bones, correct_rest_pose
from .geom_utils import bone_transform, skinning
from .mesh import _DEFAULT_COLOR, TriMesh, _Visual

FRAME_TILE = abi.CONSTANTS["MODA_ANIM_FRAME_TILE"]
BLOCK = abi.CONSTANTS["MODA_ANIM_BLOCK"]
MAX_BONES = abi.CONSTANTS["MODA_ANIM_MAX_BONES"]
RINGS, SEGMENTS = 16, 16  # the ellipsoid template's latitude bands and longitude segments
COLOR_BUDGET_BYTES = 256 << 20     # vertex_colors_frames: the `dir_src` rows of one chunk of frames stay under this


def _no_grad(what, *tensors):
    if any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what}: inputs that require grad are not implemented (mesh sequence export is evaluation "
                                  "and has no backward); pass them detached")


def _refuse_warps(what, opts):
    if getattr(opts, 'flowbw', False) or getattr(opts, 'lbs', False) or not getattr(opts, 'neudbs', True):
        raise NotImplementedError(f"{what}: flowbw / lbs warps: MoDA runs neudbs (moda.py:72-73)")


def _points(what, t, device=None):
    """(V,3) fp32 contiguous device tensor from a device tensor, or (upload) from numpy / a host tensor."""
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t, np.float32))
    _no_grad(what, t)
    if not t.is_cuda:
        if device is None:
            raise RuntimeError(f"{what} takes CUDA (ROCm) tensors; the HIP library is the only compute path")
        t = t.to(device)
    t = L.dev(t)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: expected (V, 3) points, got {tuple(t.shape)}")
    return t


def _num_frames(model):
    first = model.nerf_body_rts[0] if isinstance(model.nerf_body_rts, torch.nn.Sequential) else None
    if hasattr(first, 'vid_offset'):
        return int(np.asarray(first.vid_offset)[-1])
    if isinstance(first, torch.nn.Embedding):
        return int(first.num_embeddings)
    return None


def _frame_ids(what, model, ids, device, limit="frames"):
    """Frame ids as a (F,) int64 device tensor.  Ids given on the host (list, numpy, host tensor) are checked against the model's
    frame count; a device tensor is taken as it is (checking it would be a read-back; FrameCode reads no table through an id)."""
    if torch.is_tensor(ids) and ids.is_cuda:
        return ids.reshape(-1).long()
    host = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).reshape(-1)
    if host.size and not np.issubdtype(host.dtype, np.integer):
        raise ValueError(f"{what}: frame ids must be integers, got {host.dtype}")
    n = _num_frames(model) if limit == "frames" else limit
    if host.size and n is not None and (host.min() < 0 or host.max() >= n):
        raise ValueError(f"{what}: frame ids span [{host.min()}, {host.max()}], the model holds frames 0..{n - 1}")
    return torch.as_tensor(host.astype(np.int64)).to(device)


def _rest_pose(opts, model):
    B = int(opts.num_bones)
    if model.bones.shape[-2] != B:
        raise ValueError(f"opts.num_bones = {B}, model.bones holds {model.bones.shape[-2]}")
    return correct_bones(model, model.bones, neudbs=True)                            # geom_utils.py:1041


@torch.no_grad()
def skin_weights(opts, model, vertices):
    """The frame-independent half of warp_fw (geom_utils.py:1046-1059): gauss_mlp_skinning(vertices, embedding_xyz, bones_rst,
    rest_pose_code, nerf_skin | None, skin_aux) with bones_rst from correct_bones -> (V, B) fp32, through the fused skin MLP and
    moda_skinning_fwd.  It is also the `skins` array eval() colours the rest mesh with (train_utils.py:571-580)."""
    _refuse_warps("skin_weights", opts)
    pts = _points("skin_weights", vertices, L.dev(model.bones).device)
    bones_rst, _ = _rest_pose(opts, model)
    if pts.shape[0] == 0:
        return torch.empty((0, bones_rst.shape[-2]), device=pts.device)
    emb = model.embedding_xyz
    dskin = None
    if getattr(opts, 'nerf_skin', True):
        rest = model.rest_pose_code.weight[:1]                                       # :1049-1050
        dskin = model.nerf_skin.fused(pts[None], n_freq=emb.N_freqs, alpha=emb.alpha, code=L.dev(rest.detach()))
    return skinning(bones_rst, pts[None], dskin, model.skin_aux)[0]


@torch.no_grad()
def displaced_vertices(opts, model, vertices):
    """vertices + nerf_dis(vertices, rest_pose_code) (geom_utils.py:420-422), the points the forward blend is applied to when
    opts.nerf_dis is set; once for the whole sequence."""
    pts = _points("displaced_vertices", vertices, L.dev(model.bones).device)
    if pts.shape[0] == 0:
        return pts
    emb = model.embedding_xyz
    return pts + model.nerf_dis.fused(pts[None], n_freq=emb.N_freqs, alpha=emb.alpha,
                                      code=L.dev(model.rest_pose_code.weight[:1].detach()))[0]


def dqs_frames(dq, skin, pts, frame_splits=0):
    """moda_dqs_frames: dq (F, B, 8), skin (V, B), pts (V, 3) device tensors -> (F, V, 3): dqs_blend_skinning_chunk
    (geom_utils.py:457-493) of the same points and weights under every frame's dual quaternions.  frame_splits: how many
    workgroups share the frame tiles of one block of BLOCK vertices (0: chosen from the sizes); the result has the same bits for
    every value.  B <= MAX_BONES."""
    _no_grad("dqs_frames", dq, skin, pts)
    for t in (dq, skin, pts):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("dqs_frames takes CUDA (ROCm) tensors; the HIP library is the only compute path")
    if dq.dim() != 3 or dq.shape[2] != 8 or skin.dim() != 2 or pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"dqs_frames: expected dq (F, B, 8), skin (V, B), pts (V, 3), got {tuple(dq.shape)}, {tuple(skin.shape)}, "
                         f"{tuple(pts.shape)}")
    F, B, V = int(dq.shape[0]), int(dq.shape[1]), int(pts.shape[0])
    if skin.shape[0] != V or skin.shape[1] != B:
        raise ValueError(f"dqs_frames: skin {tuple(skin.shape)} does not match {V} points and {B} bones")
    if B < 1 or B > MAX_BONES:
        raise ValueError(f"dqs_frames: B = {B} bones, the kernel is built for 1..MAX_BONES = {MAX_BONES} (MODA_ANIM_MAX_BONES)")
    if int(frame_splits) < 0:
        raise ValueError(f"dqs_frames: frame_splits = {frame_splits}")
    q, s, p = L.dev(dq), L.dev(skin), L.dev(pts)
    out = torch.empty((F, V, 3), device=p.device, dtype=torch.float32)
    if F and V:
        L.call("moda_dqs_frames", L.ptr(q), L.ptr(s), L.ptr(p), F, V, B, int(frame_splits), L.ptr(out), L.stream())
    return out


@torch.no_grad()
def warp_fw_frames(opts, model, vertices, embedids, skin=None):
    """warp_fw (geom_utils.py:1029-1073) for all frames `embedids` (F,) at once: canonical vertices (V, 3) -> (verts (F, V, 3),
    bones (F, B, 10)), device tensors.  One nerf_body_rts(embedids) call plus correct_rest_pose gives every frame's dual
    quaternions, bone_transform the posed bones, moda_dqs_frames the vertices.  skin (V, B): the weights of
    skin_weights(opts, model, vertices) when the caller already has them.  Host embedids are checked against the model's frame
    count; nothing is read back."""
    _refuse_warps("warp_fw_frames", opts)
    dev = L.dev(model.bones).device
    pts = _points("warp_fw_frames", vertices, dev)
    _no_grad("warp_fw_frames", skin)
    ids = _frame_ids("warp_fw_frames", model, embedids, dev)
    B, F, V = int(opts.num_bones), int(ids.shape[0]), int(pts.shape[0])
    if B > MAX_BONES:
        raise ValueError(f"warp_fw_frames: B = {B} bones, moda_dqs_frames is built for at most MAX_BONES = {MAX_BONES}")
    if skin is not None and (not torch.is_tensor(skin) or tuple(skin.shape) != (V, B)):
        raise ValueError(f"warp_fw_frames: skin must be a ({V}, {B}) tensor, got {tuple(skin.shape) if torch.is_tensor(skin) else type(skin)}")
    bones_rst, bone_rts_rst = _rest_pose(opts, model)
    if F == 0:
        return torch.empty((0, V, 3), device=dev), torch.empty((0, B, 10), device=dev)
    rts = model.nerf_body_rts(ids)                                                   # (F, 1, 8B)   :1040
    rts = correct_rest_pose(opts, rts, bone_rts_rst, True).reshape(F, B, 8)          # :1042
    bones = bone_transform(bones_rst, rts, True, is_vec=True)                        # :1070
    if skin is None:
        skin = skin_weights(opts, model, pts)
    p = displaced_vertices(opts, model, pts) if getattr(opts, 'nerf_dis', False) else pts
    return dqs_frames(rts, skin, p), bones


def _cam_centres(what, rtks, F, device):
    rtks = torch.as_tensor(np.asarray(rtks, np.float32)) if not torch.is_tensor(rtks) else rtks
    _no_grad(what, rtks)
    rtks = rtks.to(device=device, dtype=torch.float32)
    if rtks.dim() != 3 or tuple(rtks.shape[1:]) != (4, 4):
        raise ValueError(f"{what}: rtks must be (F, 4, 4) = [R | T ; fx fy px py], got {tuple(rtks.shape)}")
    if rtks.shape[0] != F:
        raise ValueError(f"{what}: {rtks.shape[0]} cameras for {F} frames")
    R, T = rtks[:, :3, :3], rtks[:, :3, 3:4]
    return rtks, (-R.transpose(1, 2).matmul(T))[..., 0].contiguous()                 # train_utils.py:540-541


@torch.no_grad()
def vertex_colors_frames(model, rest_vertices, verts_frames, rtks, env_ids, budget_bytes=COLOR_BUDGET_BYTES):
    """get_vertex_colors (utils/io.py:559-582) for all frames -> (F, V, 3) fp32 in [0, 1], a device tensor: nerf_coarse at the
    REST vertices (V, 3), with the view direction normalize(verts_frames[f] - camera centre of rtks[f]), centre = -R^T t
    (train_utils.py:540-543), and the environment code env_code(env_ids[f]); clipped to [0, 1].

    env_ids (F,) is explicit: the reference passes the INDEX WITHIN THE BATCH (frame_idx=idx, train_utils.py:544), not the frame
    id, so its colours depend on how the frames were batched; pass range(F) for that behaviour or the frame ids for a
    batch-independent one.  verts_frames=None (then rtks is ignored) is the reference's view_dir=None: the fixed direction
    (0, 0, -1), F = len(env_ids).  One launch of moda_color_dirs assembles the `dir_src` rows NeRF.fused takes per sample;
    frames are taken in chunks whose rows stay under budget_bytes (F V (27 + 64) floats do not fit for a long sequence); the
    chunking changes no bit."""
    what = "vertex_colors_frames"
    coarse, emb, emb_d = model.nerf_coarse, model.embedding_xyz, model.embedding_dir
    dev = next(coarse.parameters()).device
    rest = _points(what, rest_vertices, dev)
    V = int(rest.shape[0])
    ids = _frame_ids(what, model, env_ids, dev, limit=_env_frames(model))
    F = int(ids.shape[0])
    cam = None
    if verts_frames is not None:
        if not torch.is_tensor(verts_frames) or not verts_frames.is_cuda:
            raise RuntimeError(f"{what} takes CUDA (ROCm) tensors; the HIP library is the only compute path")
        _no_grad(what, verts_frames)
        if verts_frames.dim() != 3 or verts_frames.shape[1] != V or verts_frames.shape[2] != 3:
            raise ValueError(f"{what}: verts_frames must be (F, {V}, 3), got {tuple(verts_frames.shape)}")
        if verts_frames.shape[0] != F:
            raise ValueError(f"{what}: {verts_frames.shape[0]} frames of vertices for {F} env_ids")
        verts_frames = L.dev(verts_frames)
        _, cam = _cam_centres(what, rtks, F, dev)
    out = torch.empty((F, V, 3), device=dev, dtype=torch.float32)
    if F == 0 or V == 0:
        return out
    env = L.dev(model.env_code(ids).detach()).reshape(F, -1)                         # io.py:564
    Ce, nf = int(env.shape[1]), int(emb_d.N_freqs)
    Wd = 3 * (1 + 2 * nf) + Ce
    if Wd != coarse.in_channels_dir:
        raise ValueError(f"{what}: nerf_coarse takes {coarse.in_channels_dir} direction channels, embedding_dir and env_code give {Wd}")
    win = (L._F32 * 16)(*(list(emb_d.window()) + [0.0] * (16 - nf)))
    per = max(1, int(budget_bytes) // (V * Wd * 4))
    for f0 in range(0, F, per):
        n = min(per, F - f0)
        rows = torch.empty((n * V, Wd), device=dev, dtype=torch.float32)
        L.call("moda_color_dirs", L.ptr(None if cam is None else verts_frames[f0:f0 + n]), L.ptr(None if cam is None else cam[f0:f0 + n]),
               L.ptr(env[f0:f0 + n]), n, V, nf, win, Ce, L.ptr(rows), L.stream())
        xyz = rest[None].expand(n, V, 3).reshape(-1, 3)
        rgb = coarse.fused(xyz, n_freq=emb.N_freqs, alpha=emb.alpha, dir_src=rows)[:, :3]           # io.py:580
        out[f0:f0 + n] = rgb.reshape(n, V, 3).clamp_(0, 1)                            # :581
    return out


def _env_frames(model):
    ec = getattr(model, 'env_code', None)
    if hasattr(ec, 'vid_offset'):
        return int(np.asarray(ec.vid_offset)[-1])
    if isinstance(ec, torch.nn.Embedding):
        return int(ec.num_embeddings)
    return None


# ---- bones as ellipsoids, skin colours --------------------------------------------------------------------------------------------
def uv_sphere(rings=RINGS, segments=SEGMENTS):
    """The unit UV sphere of this module, by rule: vertex 0 = (0, 0, 1); then for ring i = 1 .. rings - 1 and segment j = 0 ..
    segments - 1 the point (sin t cos p, sin t sin p, cos t), t = pi i / rings, p = 2 pi j / segments, at index 1 + (i - 1)
    segments + j; last vertex (0, 0, -1).  Faces, counter-clockwise seen from outside: a fan around each pole and two triangles
    per quad between neighbouring rings.  2 + (rings - 1) segments vertices, 2 segments (rings - 1) faces, closed.
    -> (vertices (Nv, 3) float64, faces (Nf, 3) int64), numpy.  NOT trimesh.creation.uv_sphere: counts are not claimed equal."""
    if rings < 2 or segments < 3:
        raise ValueError(f"uv_sphere: rings >= 2 and segments >= 3, got {rings}, {segments}")
    t = np.pi * np.arange(1, rings) / rings
    p = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(t)[:, None] * np.cos(p)[None], np.sin(t)[:, None] * np.sin(p)[None],
                     np.broadcast_to(np.cos(t)[:, None], (rings - 1, segments))], -1).reshape(-1, 3)
    verts = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]], 0)
    idx = lambda i, j: 1 + (i - 1) * segments + (j % segments)
    south = len(verts) - 1
    faces = []
    for j in range(segments):
        faces.append((0, idx(1, j), idx(1, j + 1)))
    for i in range(1, rings - 1):
        for j in range(segments):
            a, b, c, d = idx(i, j), idx(i, j + 1), idx(i + 1, j), idx(i + 1, j + 1)
            faces.append((a, c, d))
            faces.append((a, d, b))
    for j in range(segments):
        faces.append((south, idx(rings - 1, j + 1), idx(rings - 1, j)))
    return verts, np.asarray(faces, np.int64)


def default_palette(n):
    """n bone colours (n, 3) uint8 by rule, a fixed hue walk: colour i has hue frac(i * 0.618033988749895) (the golden-ratio
    conjugate: neighbouring indices land far apart on the colour wheel), saturation 0.55 + 0.15 (i mod 3), value 0.95, through
    colorsys.hsv_to_rgb, each channel rounded to the nearest of 0..255.  Not the reference's label_colormap."""
    out = np.empty((int(n), 3), np.uint8)
    for i in range(int(n)):
        rgb = colorsys.hsv_to_rgb((i * 0.618033988749895) % 1.0, 0.55 + 0.15 * (i % 3), 0.95)
        out[i] = [int(round(255 * c)) for c in rgb]
    return out


def _palette(what, palette, B, device):
    """-> (host (B,3) uint8 | None, device (B,3) fp32 in 0..255)."""
    if palette is None:
        host = default_palette(B)
        return host, L.const_tensor(("animate_palette", B), device, lambda: host.astype(np.float32))
    if torch.is_tensor(palette):
        _no_grad(what, palette)
        pal = palette.to(device=device, dtype=torch.float32)
    else:
        pal = torch.as_tensor(np.asarray(palette, np.float32)).to(device)
    if pal.dim() != 2 or pal.shape[1] != 3 or pal.shape[0] < B:
        raise ValueError(f"{what}: palette must be (>= {B}, 3) colours in 0..255, got {tuple(pal.shape)}")
    return None, pal[:B].contiguous()


def skin_colors(skin, palette=None):
    """(palette[None] * skin[..., None]).sum(1) (train_utils.py:582-590): skin (V, B) device tensor, palette (>= B, 3) colours in
    0..255 (numpy or tensor; None: default_palette(B)) -> (V, 3) fp32 in the palette's units, a device tensor."""
    _no_grad("skin_colors", skin)
    if not torch.is_tensor(skin) or not skin.is_cuda:
        raise RuntimeError("skin_colors takes CUDA (ROCm) tensors; the HIP library is the only compute path")
    if skin.dim() != 2 or skin.shape[1] < 1:
        raise ValueError(f"skin_colors: skin must be (V, B), got {tuple(skin.shape)}")
    s = L.dev(skin)
    V, B = int(s.shape[0]), int(s.shape[1])
    _, pal = _palette("skin_colors", palette, B, s.device)
    out = torch.empty((V, 3), device=s.device, dtype=torch.float32)
    if V:
        L.call("moda_skin_colors", L.ptr(s), L.ptr(pal), V, B, L.ptr(out), L.stream())
    return out


def bone_ellipsoids(bones, len_max, palette=None):
    """save_bones (utils/io.py:51-78) as one instancing launch: bones (F, B, 10) (or (B, 10)) device tensor = [centre |
    quaternion, real first | log scale] -> (verts (F, B Nv, 3) fp32, faces (B Nf, 3) int32, colors (B Nv, 3) uint8), device
    tensors; faces and colours are the same for every frame.  Every bone is the template `uv_sphere()` of radius len_max / 20
    (len_max: a number, or a 0-dim device tensor, which is not read back), divided by exp(scale), rotated by the normalised
    quaternion and moved to the centre; bone b takes palette[b] (None: default_palette(B))."""
    _no_grad("bone_ellipsoids", bones, len_max, palette)
    if not torch.is_tensor(bones) or not bones.is_cuda:
        raise RuntimeError("bone_ellipsoids takes CUDA (ROCm) tensors; the HIP library is the only compute path")
    if bones.dim() == 2:
        bones = bones[None]
    if bones.dim() != 3 or bones.shape[2] != 10 or bones.shape[1] < 1:
        raise ValueError(f"bone_ellipsoids: bones must be (F, B, 10), got {tuple(bones.shape)}")
    b = L.dev(bones)
    F, B = int(b.shape[0]), int(b.shape[1])
    dev = b.device
    tv, tf = uv_sphere()
    Nv = len(tv)
    unit = L.const_tensor(("animate_sphere", RINGS, SEGMENTS), dev, lambda: tv.astype(np.float32))
    radius = (len_max.to(device=dev, dtype=torch.float32) if torch.is_tensor(len_max) else float(len_max)) / 20     # io.py:54
    tmpl = (unit * radius).contiguous()
    key = ("animate_sphere_faces", RINGS, SEGMENTS, B, str(dev))
    faces = L._CONST.get(key)
    if faces is None:
        faces = torch.as_tensor((tf[None] + Nv * np.arange(B)[:, None, None]).reshape(-1, 3).astype(np.int32)).to(dev)
        L._CONST[key] = faces
    _, pal = _palette("bone_ellipsoids", palette, B, dev)
    colors = pal.to(torch.uint8)[:, None].expand(B, Nv, 3).reshape(-1, 3).contiguous()             # io.py:75-77
    verts = torch.empty((F, B * Nv, 3), device=dev, dtype=torch.float32)
    if F:
        L.call("moda_bone_ellipsoids", L.ptr(b), F * B, L.ptr(tmpl), Nv, L.ptr(verts), L.stream())
    return verts, faces, colors


# ---- the OBJ files ----------------------------------------------------------------------------------------------------------------
def write_obj(path, vertices, faces, colors=None):
    """A plain host function: `v x y z[ r g b]` lines (9 significant digits: an fp32 value survives the round trip; colours as
    0..1 floats, given as (V, 3|4) uint8 or as floats already in 0..1), then 1-based `f a b c` lines."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"write_obj: faces index [{f.min()}, {f.max()}], the mesh has {len(v)} vertices")
    cols = [v]
    if colors is not None:
        c = np.asarray(colors)
        c = c[:, :3].astype(np.float64) / 255.0 if c.dtype == np.uint8 else c[:, :3].astype(np.float64)
        if len(c) != len(v):
            raise ValueError(f"write_obj: {len(c)} colours for {len(v)} vertices")
        cols.append(c)
    with open(path, "w") as fh:
        np.savetxt(fh, np.concatenate(cols, 1), fmt="v" + " %.9g" * (3 * len(cols)))
        np.savetxt(fh, f + 1, fmt="f %d %d %d")


def read_obj(path):
    """What write_obj wrote -> (vertices (V,3) float64, faces (F,3) int64 0-based, colors (V,3) float64 in 0..1 | None)."""
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if p and p[0] == "v":
                v.append([float(x) for x in p[1:]])
            elif p and p[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
    v = np.asarray(v, np.float64).reshape(len(v), -1)
    return v[:, :3], np.asarray(f, np.int64).reshape(-1, 3), (v[:, 3:6] if v.shape[1] >= 6 else None)


class _DeviceVisual(_Visual):
    """TriMesh.visual whose colours lie on the device until the host asks for them (`_colors`, which _Visual, TriMesh.copy and
    render_mesh read, fetches them on first access)."""

    def __init__(self, mesh, colors_t):
        self._colors_t, self._host = colors_t, None
        super().__init__(mesh)

    @property
    def _colors(self):
        if self._host is None and self._colors_t is not None:
            rgb = self._colors_t.detach().cpu().numpy().astype(np.uint8)
            self._host = np.concatenate([rgb, np.full((len(rgb), 1), 255, np.uint8)], 1)
        return self._host

    @_colors.setter
    def _colors(self, c):
        self._host = c
        if c is not None:
            self._colors_t = None


class MeshSequence:
    """What export_sequence returns, all device tensors: verts (F, V, 3) fp32, faces (Nf, 3) int32, colors (F, V, 3) or (V, 3)
    uint8 (one set for every frame: the rest surface colour, opts.ce_color), bones (F, B, 10), bone_mesh = (verts (F, B Nv, 3),
    faces, colors) of bone_ellipsoids, rest_skin_colors (V, 3) uint8 | None, rtk (F, 4, 4); and the rest pose: rest_verts
    (V, 3), rest_colors (V, 3) uint8, bone_rest_mesh."""

    def __init__(self, verts, faces, colors, bones, bone_mesh, rest_skin_colors, rtk, rest_verts, rest_colors, bone_rest_mesh):
        self.verts, self.faces, self.colors, self.bones, self.bone_mesh = verts, faces, colors, bones, bone_mesh
        self.rest_skin_colors, self.rtk = rest_skin_colors, rtk
        self.rest_verts, self.rest_colors, self.bone_rest_mesh = rest_verts, rest_colors, bone_rest_mesh

    def __len__(self):
        return int(self.verts.shape[0])

    def frame(self, i):
        """Frame i as a TriMesh over device views (render_mesh and eval_mesh take it as it is); nothing is copied until the
        host attributes (.vertices, .faces, .visual.vertex_colors) are touched."""
        i = range(len(self))[i]
        m = TriMesh(self.verts[i], self.faces)
        m.visual = _DeviceVisual(m, self.colors[i] if self.colors.dim() == 3 else self.colors)
        return m

    def render(self, image_hw, **kwargs):
        """seq_render.render_sequence(self, image_hw, **kwargs): every frame drawn from one of render_vis.py's viewpoints."""
        from .seq_render import render_sequence
        return render_sequence(self, image_hw, **kwargs)

    def save(self, dir, names, frame_numbers):
        """The reference's file set (extract.py:24-53) under `dir`: mesh-rest.obj, mesh-rest-skin.obj, bone-rest.obj, and per
        frame i <names[i]>-mesh-%05d.obj, <names[i]>-bone-%05d.obj, <names[i]>-cam-%05d.txt (np.savetxt of the 4 x 4) with
        frame_numbers[i].  names: one sequence name for all frames, or one per frame.  The only place the device is read back:
        one copy per array.  -> the list of paths written."""
        F = len(self)
        names = [names] * F if isinstance(names, str) else list(names)
        nums = [int(n) for n in frame_numbers]
        if len(names) != F or len(nums) != F:
            raise ValueError(f"MeshSequence.save: {len(names)} names and {len(nums)} frame numbers for {F} frames")
        os.makedirs(dir, exist_ok=True)
        host = lambda t: None if t is None else t.detach().cpu().numpy()
        verts, faces, colors, rtk = host(self.verts), host(self.faces), host(self.colors), host(self.rtk)
        bverts, bfaces, bcolors = (host(t) for t in self.bone_mesh)
        rest_v, rest_c, skin_c = host(self.rest_verts), host(self.rest_colors), host(self.rest_skin_colors)
        brest = host(self.bone_rest_mesh[0])
        paths = []

        def put(name, *a):
            paths.append(os.path.join(dir, name))
            write_obj(paths[-1], *a)
        put("mesh-rest.obj", rest_v, faces, rest_c)
        if skin_c is not None:
            put("mesh-rest-skin.obj", rest_v, faces, skin_c)
        put("bone-rest.obj", brest[0], bfaces, bcolors)
        for i in range(F):
            put("%s-mesh-%05d.obj" % (names[i], nums[i]), verts[i], faces, colors[i] if colors.ndim == 3 else colors)
            put("%s-bone-%05d.obj" % (names[i], nums[i]), bverts[i], bfaces, bcolors)
            paths.append(os.path.join(dir, "%s-cam-%05d.txt" % (names[i], nums[i])))
            np.savetxt(paths[-1], rtk[i])
        return paths


def _to_u8(t):
    return (t * 255).clamp_(0, 255).to(torch.uint8)


@torch.no_grad()
def export_sequence(opts, model, mesh_rest, embedids, rtks, env_ids=None, palette=None, len_max=None):
    """The mesh sequence of eval(dynamic_mesh=True) with queryfw (train_utils.py:522-593) for the frames `embedids` (F,) and their
    cameras rtks (F, 4, 4): mesh_rest (a TriMesh; its device vertices and faces are used as they are) warped to every frame,
    the posed and the rest bones as ellipsoids, the rest mesh coloured by its skinning weights -> MeshSequence.

    Vertex colours: with opts.ce_color (the default) every frame carries the rest mesh's colours (:535-537); otherwise
    vertex_colors_frames with env_ids (None: range(F), the reference's index within the batch).  len_max (the ellipsoids are
    len_max / 20 in radius): None takes the largest extent of the rest vertices (extract.py:28), on the device.  The skinning
    weights are evaluated once and serve the warp and the skin colours."""
    _refuse_warps("export_sequence", opts)
    if 'flowbw' in getattr(model, 'nerf_models', {}) or 'flowfw' in getattr(model, 'nerf_models', {}):
        raise NotImplementedError("export_sequence: the flow warps are not implemented (MoDA runs neudbs)")
    dev = L.dev(model.bones).device
    rest = _points("export_sequence", mesh_rest.vertices_t, dev)
    faces = L.dev(mesh_rest.faces_t, torch.int32)
    ids = _frame_ids("export_sequence", model, embedids, dev)
    F, V = int(ids.shape[0]), int(rest.shape[0])
    rtk, _ = _cam_centres("export_sequence", rtks, F, dev)
    if V == 0:
        raise ValueError("export_sequence: the rest mesh has no vertices")
    skin = skin_weights(opts, model, rest)
    verts, bones = warp_fw_frames(opts, model, rest, ids, skin=skin)
    host_colors = getattr(mesh_rest.visual, '_colors', None)             # not the property: it would copy the vertices out
    if host_colors is None or len(host_colors) != V:
        host_colors = np.tile(np.asarray(_DEFAULT_COLOR, np.uint8), (V, 1))
    rest_colors = torch.as_tensor(np.ascontiguousarray(host_colors[:, :3])).to(dev)
    if getattr(opts, 'ce_color', True):
        colors = rest_colors
    else:
        colors = _to_u8(vertex_colors_frames(model, rest, verts, rtk, np.arange(F) if env_ids is None else env_ids))
    if len_max is None:
        len_max = (rest.max(0).values - rest.min(0).values).max()
    bones_rst, _ = _rest_pose(opts, model)
    return MeshSequence(verts, faces, colors, bones, bone_ellipsoids(bones, len_max, palette),
                        skin_colors(skin, palette).clamp_(0, 255).to(torch.uint8), rtk, rest, rest_colors,
                        bone_ellipsoids(bones_rst[None], len_max, palette))
