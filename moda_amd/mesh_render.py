"""Mesh drawing on the GPU: the third thing the reference does with a mesh, after extracting (mesh.py) and scoring
(mesh_eval.py) it.  The kernels are moda_amd/csrc/raster_kernels.hip: a tiled hard rasteriser that restates the reference's
soft_rasterize kernel in the one configuration MoDA uses (sigma_val 1e-12, hard aggregation; nnutils/moda.py:469-471), and an
attribute pass for any number of channels.

    rasterize / interpolate      visibility (face index, barycentrics, depth, cover mask) once per view, attributes from it
    render_dp                    nnutils/moda.py:931-1022: random views of the DensePose surface, all channels from ONE rasterize
    render_mesh                  what scripts/visualize/render_vis.py:324-335, 444-447, 470-490 asks of pyrender: colour, depth
                                 and silhouette of a mesh under the (4,4) camera the reference writes

`moda_amd.soft_renderer` and `moda_amd.geom_utils.render_color / render_flow` put the reference's names on top of these.
Forward only: every reference call site runs under no_grad or in a script, and inputs that require grad are refused."""
import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from . import abi

_REC_DOUBLES, _BOX_INTS = abi.CONSTANTS["MODA_RASTER_REC_DOUBLES"], abi.CONSTANTS["MODA_RASTER_BOX_INTS"]


def _faces_arg(faces, B, what):
    """(F,3) or (B,F,3) integer tensor -> (int32 contiguous device tensor, faces_per_view flag, F)."""
    if not torch.is_tensor(faces):
        raise TypeError(f"{what}: expected a tensor of faces, got {type(faces).__name__}")
    if faces.dtype.is_floating_point or faces.dtype == torch.bool:
        raise TypeError(f"{what}: faces must be an integer tensor, got {faces.dtype}")
    if faces.dim() not in (2, 3) or faces.shape[-1] != 3 or faces.shape[-2] < 1:
        raise ValueError(f"{what}: expected faces (F,3) or (B,F,3) with F >= 1, got {tuple(faces.shape)}")
    if faces.dim() == 3 and faces.shape[0] != B:
        raise ValueError(f"{what}: faces for {faces.shape[0]} views, vertices for {B}")
    return L.dev(faces, torch.int32), int(faces.dim() == 3), int(faces.shape[-2])


def _check_sizes(B, S, Fn, what):
    if S < 1 or S > 32768:
        raise ValueError(f"{what}: image_size {S} outside 1 .. 32768")
    if B * S * S >= 2 ** 31 or B * Fn >= 2 ** 31:
        raise ValueError(f"{what}: B*S*S = {B * S * S} or B*F = {B * Fn} exceeds int32 indices")


def _forward_only(what, *tensors):
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what}: gradients are not implemented (the rasteriser is forward only, as every call site "
                                  "of the reference is); call it under torch.no_grad() or detach the inputs")


def rasterize(verts, faces, image_size, near=1, far=100, binned=True, check_finite=True):
    """verts (B,V,3) fp32 on the device: x, y in NDC (y up; pixel (row, col) has its centre at x = (2 col + 1 - S) / S,
    y = (S - 1 - 2 row) / S) and z the depth that the near / far test and the 1/z weights see; faces (F,3) shared by the views
    or (B,F,3), any integer dtype.  Both windings are drawn.
    -> face_idx (B,S,S) int32, -1 where nothing is drawn; bary (B,S,S,3) fp32, the clipped and renormalised barycentrics of the
    winning face; zbuf (B,S,S) fp32, its depth 1 / sum(bary_k / z_k), 0 where nothing is drawn; alpha (B,S,S) fp32, 1 where any
    face covers the pixel centre, INCLUDING faces outside [near, far] (the reference takes alpha before its depth test).
    The nearest face wins, the lowest face index among equal depths.  binned=False sends every face to every tile: the same
    bits, slower (kept for the tests).
    check_finite: the vertices are tested for NaN / inf and a ValueError is raised, which reads one flag back from the device:
    the call then synchronises and cannot be captured into a graph (the C entries themselves read nothing back).  With
    check_finite=False nothing is read back; faces with a non-finite corner then draw nothing or garbage depths, never out
    of bounds."""
    if not torch.is_tensor(verts):
        raise TypeError(f"rasterize: expected a tensor of vertices, got {type(verts).__name__}")
    if verts.dim() != 3 or verts.shape[-1] != 3 or verts.shape[0] < 1 or verts.shape[1] < 1:
        raise ValueError(f"rasterize: expected vertices (B,V,3) with B, V >= 1, got {tuple(verts.shape)}")
    _forward_only("rasterize", verts)
    B, V, S = int(verts.shape[0]), int(verts.shape[1]), int(image_size)
    v = L.dev(verts.detach())
    f, per_view, Fn = _faces_arg(faces, B, "rasterize")
    _check_sizes(B, S, Fn, "rasterize")
    if check_finite and not bool(torch.isfinite(v).all()):                    # the one read-back of the call
        raise ValueError("rasterize: non-finite coordinate in the vertices")
    dev = v.device
    rec = torch.empty((B * Fn, _REC_DOUBLES), dtype=torch.float64, device=dev)
    box = torch.empty((B * Fn, _BOX_INTS), dtype=torch.int32, device=dev)
    face_idx = torch.empty((B, S, S), dtype=torch.int32, device=dev)
    bary = torch.empty((B, S, S, 3), dtype=torch.float32, device=dev)
    zbuf = torch.empty((B, S, S), dtype=torch.float32, device=dev)
    alpha = torch.empty((B, S, S), dtype=torch.float32, device=dev)
    L.call("moda_raster_fwd", L.ptr(v), L.ptr(f), per_view, B, V, Fn, S, float(near), float(far), int(bool(binned)), L.ptr(rec),
           L.ptr(box), L.ptr(face_idx), L.ptr(bary), L.ptr(zbuf), L.ptr(alpha), L.stream())
    return face_idx, bary, zbuf, alpha


def interpolate(attrs, faces, face_idx, bary, background=0):
    """attrs (B,V,C) fp32 vertex attributes, faces as given to rasterize, face_idx / bary from it -> (B,C,S,S) fp32:
    sum_k bary_k * attrs[faces[face_idx][k]], `background` (a number, or C numbers) where face_idx is -1.  Any C; a channel's
    bits do not depend on the channels beside it."""
    if not torch.is_tensor(attrs) or attrs.dim() != 3 or attrs.shape[-1] < 1 or attrs.shape[1] < 1:
        raise ValueError(f"interpolate: expected attributes (B,V,C), got {tuple(getattr(attrs, 'shape', ()))}")
    _forward_only("interpolate", attrs, bary)
    B, V, C = (int(s) for s in attrs.shape)
    a = L.dev(attrs.detach())
    f, per_view, Fn = _faces_arg(faces, B, "interpolate")
    fi, w = L.dev(face_idx, torch.int32), L.dev(bary)
    if fi.dim() != 3 or fi.shape[0] != B or fi.shape[1] != fi.shape[2] or tuple(w.shape) != tuple(fi.shape) + (3,):
        raise ValueError(f"interpolate: face_idx {tuple(fi.shape)} / bary {tuple(w.shape)} are not (B,S,S) / (B,S,S,3) for B = {B}")
    S = int(fi.shape[1])
    _check_sizes(B, S, Fn, "interpolate")
    bg = None
    if torch.is_tensor(background):
        bg = L.dev(background.detach()).reshape(-1)
        bg = bg.expand(C).contiguous() if bg.numel() == 1 else bg
    else:
        vals = np.asarray(background, np.float32).reshape(-1)
        vals = np.repeat(vals, C) if vals.size == 1 else vals
        if vals.any():
            bg = L.const_tensor(("raster_bg", tuple(float(x) for x in vals)), a.device, lambda: torch.as_tensor(vals.copy()))
    if bg is not None and bg.numel() != C:
        raise ValueError(f"interpolate: {bg.numel()} background values for {C} channels")
    out = torch.empty((B, C, S, S), dtype=torch.float32, device=a.device)
    L.call("moda_raster_interp", L.ptr(a), L.ptr(f), per_view, L.ptr(fi), L.ptr(w), L.ptr(bg), B, V, Fn, C, S, L.ptr(out),
           L.stream())
    return out


# ---- render_dp (nnutils/moda.py:931-1022) ------------------------------------------------------------------------------------
def axis_angle_to_matrix(axis_angle):
    """pytorch3d.transforms.axis_angle_to_matrix from its published closed form: the unit quaternion
    (cos(a/2), axis * sin(a/2)) with sin(a/2)/a taken from its series below |a| = 1e-6, then the standard rotation matrix
    scaled by 2/|q|^2."""
    angles = torch.norm(axis_angle, p=2, dim=-1, keepdim=True)
    half = angles * 0.5
    small = angles.abs() < 1e-6
    s = torch.where(small, 0.5 - (angles * angles) / 48, torch.sin(half) / torch.where(small, torch.ones_like(angles), angles))
    q = torch.cat([torch.cos(half), axis_angle * s], -1)
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def resized_crop(img, top, left, height, width, size):
    """torchvision.transforms.functional.resized_crop for a (C,H,W) tensor: the window (zero-padded where it leaves the
    image) resized bilinearly (half-pixel centres, no antialiasing) to `size`."""
    C, H, W = img.shape
    t0, l0, t1, l1 = max(top, 0), max(left, 0), min(top + height, H), min(left + width, W)
    crop = img.new_zeros((C, height, width))
    if t1 > t0 and l1 > l0:
        crop[:, t0 - top:t1 - top, l0 - left:l1 - left] = img[:, t0:t1, l0:l1]
    return F.interpolate(crop[None], size=tuple(size), mode="bilinear", align_corners=False)[0]


def dp_cameras(near_far, device, bs, img_size=256, focal=2, std_rot=6.28, std_dep=0.5):
    """The random views of render_dp (moda.py:949-971), np.random drawn in the reference's order (depth, then rotation).
    -> (Rmat (bs,3,3), Tmat (bs,3), K (bs,4), rtk (bs,4,4), d_mean)."""
    d_mean = near_far.mean()
    dep_rand = 1 + np.random.normal(0, std_dep, bs)
    dep_rand = torch.Tensor(dep_rand).to(device)
    d_obj = d_mean * dep_rand
    d_obj = torch.max(d_obj, 1.2 * 1 / 3 * d_mean)
    rot_rand = np.random.normal(0, std_rot, (bs, 3))
    rot_rand = torch.Tensor(rot_rand).to(device)
    Rmat = axis_angle_to_matrix(rot_rand)
    Tmat = torch.cat([torch.zeros(bs, 2).to(device), d_obj[:, None]], -1)
    K = torch.Tensor([[focal, focal, 0, 0]]).to(device).repeat(bs, 1)
    Kimg = torch.Tensor([[focal * img_size / 2., focal * img_size / 2., img_size / 2., img_size / 2.]]).to(device).repeat(bs, 1)
    rtk = torch.zeros(bs, 4, 4).to(device)
    rtk[:, :3, :3] = Rmat
    rtk[:, :3, 3] = Tmat
    rtk[:, 3, :] = Kimg
    return Rmat, Tmat, K, rtk, d_mean


def dp_crops(rendered, crop_size=112):
    """moda.py:999-1021: per view the box of the non-zero pixels, resized_crop to 50 x 50, mask_aug, then all views resized to
    crop_size and normalised over the channels."""
    from .geom_utils import mask_aug
    crops = []
    for i in range(rendered.shape[0]):
        mask = (rendered[i].max(0)[0] > 0).cpu().numpy()
        indices = np.where(mask > 0)
        xid, yid = indices[1], indices[0]
        if len(xid) == 0:
            raise ValueError(f"render_dp: view {i} shows nothing of the surface")     # the reference fails on xid.max() here
        center = ((xid.max() + xid.min()) // 2, (yid.max() + yid.min()) // 2)
        length = (int((xid.max() - xid.min()) * 1. // 2), int((yid.max() - yid.min()) * 1. // 2))
        left, top, w, h = [center[0] - length[0], center[1] - length[1], length[0] * 2, length[1] * 2]
        crop = resized_crop(rendered[i], int(top), int(left), max(int(h), 1), max(int(w), 1), (50, 50))
        crops.append(mask_aug(crop))
    crops = torch.stack(crops, 0)
    crops = F.interpolate(crops, (crop_size, crop_size), mode='bilinear')
    return F.normalize(crops, 2, 1)


@torch.no_grad()
def render_dp(dp_verts_unit, dp_faces, dp_embed, near_far, device, mesh_renderer, bs):
    """nnutils/moda.py:931-1022 (a static method of the reference's model): `bs` random views of the DensePose surface
    -> (features (bs, embed_dim, 112, 112), rtk (bs,4,4)).  The reference renders ceil(embed_dim / 3) times, three channels a
    time; here the views are rasterised ONCE and all embed_dim channels are interpolated from that (bit-identical to the
    3-wide renders: a channel's arithmetic does not depend on its neighbours).  Random draws: np.random, in the reference's
    order (depths, rotations, then mask_aug's per view)."""
    from .geom_utils import obj_to_cam, pinhole_cam, render_color
    num_verts, embed_dim = dp_embed.shape
    Rmat, Tmat, K, rtk, d_mean = dp_cameras(near_far, device, bs)
    verts = dp_verts_unit / 3 * d_mean
    verts = verts[None].repeat(bs, 1, 1)
    verts = obj_to_cam(verts, Rmat, Tmat)
    verts = pinhole_cam(verts, K)
    rendered = render_color(mesh_renderer, verts, dp_faces, dp_embed[None].repeat(bs, 1, 1), texture_type='vertex')
    return dp_crops(rendered[:, :embed_dim]), rtk


# ---- render_mesh (scripts/visualize/render_vis.py) -----------------------------------------------------------------------------
def vertex_normals(verts, faces):
    """Area-weighted vertex normals of a (V,3) / (F,3) mesh: face cross products summed onto their corners, normalised."""
    f = faces.long()
    v0, v1, v2 = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    fn = torch.cross(v1 - v0, v2 - v0, dim=-1)
    n = torch.zeros_like(verts)
    for k in range(3):
        n.index_add_(0, f[:, k], fn)
    return F.normalize(n, dim=-1, eps=1e-12)


@torch.no_grad()
def render_mesh(mesh, rtk, image_size, smooth=True, colors=None, znear=1e-3, zfar=1000.0):
    """Colour, depth and silhouette of a mesh as scripts/visualize/render_vis.py:324-335, 444-447, 470-490 obtains them from
    pyrender with its perspective camera.  mesh: a TriMesh, or (vertices (V,3), faces (F,3)); colours from
    mesh.visual.vertex_colors or `colors` ((V,3|4), 0..255).  rtk (4,4): [R|T] over [fx, fy, px, py] in pixels.
    Vertices go to the camera frame (obj_to_cam), then to pixels u = fx X/Z + px, v = fy Y/Z + py (v down); depth is the
    perspective-correct camera Z of the nearest face in (znear, zfar) at each pixel centre (u, v) = (col + 0.5, row + 0.5).
    Shading: Lambert, 0.6 * colour * (0.4 ambient + |n . view axis|) clipped to 255, with interpolated area-weighted vertex
    normals (smooth) or face normals, both sides lit (the reference skips face culling).  No pixel parity with pyrender is
    claimed: OpenGL's fill rule and its material model differ.
    -> color (S,S,3) uint8 with color[0,0] = 0 (render_vis.py:494), depth (S,S) fp32 (0 = nothing), sil = depth > 0."""
    from .geom_utils import obj_to_cam
    if isinstance(mesh, (tuple, list)):
        verts, faces = mesh[0], mesh[1]
    else:
        verts, faces = mesh.vertices_t, mesh.faces_t
        if colors is None and mesh.visual._colors is not None:
            colors = mesh.visual.vertex_colors
    if not (torch.is_tensor(verts) and torch.is_tensor(faces)):
        raise TypeError("render_mesh: expected device tensors of vertices and faces (or a TriMesh)")
    verts = L.dev(verts.detach()).reshape(-1, 3)
    faces = L.dev(faces, torch.int32).reshape(-1, 3)
    dev, S = verts.device, int(image_size)
    rtk = torch.as_tensor(np.asarray(rtk.detach().cpu() if torch.is_tensor(rtk) else rtk, np.float32)).reshape(4, 4).to(dev)
    cam = obj_to_cam(verts[None], rtk[None, :3, :3], rtk[None, :3, 3])[0]
    fx, fy, px, py = rtk[3]
    z = cam[:, 2]
    zs = torch.where(z.abs() < 1e-12, torch.full_like(z, 1e-12), z)
    u, v = fx * cam[:, 0] / zs + px, fy * cam[:, 1] / zs + py
    ndc = torch.stack([u * (2.0 / S) - 1.0, -(v * (2.0 / S) - 1.0), z], -1)
    # a vertex behind the camera would wrap around under the division: such faces are dropped, not clipped
    keep = (z[faces.long()] > 0).all(-1)
    depth = torch.zeros((S, S), dtype=torch.float32, device=dev)
    color = torch.zeros((S, S, 3), dtype=torch.uint8, device=dev)
    if int(keep.sum()) == 0:
        return color, depth, depth > 0
    fk = faces[keep].contiguous()
    face_idx, bary, zbuf, _ = rasterize(ndc[None], fk, S, near=znear, far=zfar)
    depth = zbuf[0]
    sil = depth > 0
    if colors is None:
        base = torch.full((verts.shape[0], 3), 102.0, device=dev)
    else:
        base = torch.as_tensor(np.asarray(colors.detach().cpu() if torch.is_tensor(colors) else colors, np.float32))[:, :3].to(dev)
    base = torch.floor(0.6 * base)                                            # render_vis.py:335, through uint8
    if smooth:
        attrs = torch.cat([base, vertex_normals(cam, fk)], -1)
        img = interpolate(attrs[None], fk, face_idx, bary)[0]
        rgb, n = img[:3], F.normalize(img[3:6], dim=0, eps=1e-12)
        lambert = n[2].abs()
    else:
        rgb = interpolate(base[None], fk, face_idx, bary)[0]
        f = fk.long()
        fn = F.normalize(torch.cross(cam[f[:, 1]] - cam[f[:, 0]], cam[f[:, 2]] - cam[f[:, 0]], dim=-1), dim=-1, eps=1e-12)
        lambert = fn[face_idx[0].clamp(min=0).long(), 2].abs()
    shade = (rgb * (0.4 + lambert)[None]).clamp(0.0, 255.0)
    color = torch.where(sil[None], shade, torch.zeros_like(shade)).permute(1, 2, 0).to(torch.uint8)
    color[0, 0, :] = 0
    return color, depth, sil
