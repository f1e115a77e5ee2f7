"""Mesh sequence rendering, device-resident: the step of the reference's result pipeline between extract.py and ffmpeg,
scripts/visualize/render_vis.py:246-511, for ALL frames of a MeshSequence in one call.  The five runs of scripts/render_result.sh
(--freeze; --vp -1 --vis_bones; --vp 0, 1, 2) and the error-coloured runs of scripts/eval/run_eval.sh are arguments of
`render_sequence`.

Five stages, the HIP entries of include/moda_hip_seqvis.h (csrc/seqvis_kernels.hip) around the rasteriser moda_raster_fwd:
    cams      every frame's viewpoint camera in float64, one launch for the sequence (moda_seqvis_cams)
    project   obj_to_cam, pixels, NDC and the per-view face lists: a face with a corner at Z <= 0 becomes (-1, -1, -1), which the
              rasteriser skips -- nothing is compacted, nothing read back (moda_seqvis_project)
    records   per (frame, vertex) one 32-byte record: base colour and the area-weighted camera-frame normal, summed over a
              vertex -> (face, corner) CSR in ascending face order (moda_seqvis_records)
    shade     Lambert shading of the body and, under `bones`, of a second raster pass over seq.bone_mesh, composited, overlaid
              on the input frame, cropped to H x W (moda_seqvis_shade)
    resize    bilinear to (h, out_width) (moda_seqvis_resize)
Frames go through project .. resize in chunks under `budget_bytes`; a frame's bits do not depend on the chunking.  Nothing is
read back: `SeqRender.status` is a device word, `SeqRender.save_ctrajs` the only copy to the host.  After one eager call a call
with the same shapes can be captured with torch.cuda.graph on one stream; a replay follows vertices and cameras rewritten in place.

What is and is not pinned.  pyrender, trimesh and cv2 are absent, so the reference script cannot run: the viewpoint block is
RESTATED (tests/seqvis_numpy.py) and unpinned; Rodrigues is pinned to scipy, the plasma table and its lookup rule to matplotlib,
obj_to_cam and the pixel projection to oracle/torch_ref.py.  No pixel parity with pyrender / OpenGL is claimed, as for
mesh_render.render_mesh, whose Lambert rule this module keeps.  Stated departures:
  * The reference passes focal[0] for both focal lengths to pyrender (:471-476) and writes it twice into ctrajs; this module
    renders with the row's own fx, fy, as render_mesh does, and `ctrajs` reports what it rendered with.
  * The vertex mean of vp 1 / 2 is a float64 sum in a fixed order (the reference: torch's fp32 mean).
  * gray_color: the reference sets the colours to 128 on loading (:152) and line :335 then scales them like any colour, so the
    base colour is floor(0.6 * 128) = 76.
  * Error colours: plasma(5 * vertex_error) as bytes (matplotlib's bytes=True); what trimesh then does to float colours is
    unpinned.  They are not scaled by 0.6 (the reference assigns them after :335).
  * Compositing: the reference marks the body alpha 254 (:184) and leaves the blend to pyrender; here the bone colour wins where
    it is nearer or the body absent, the body colour stands alone where no bone lies behind it, and otherwise the result is
    mesh_opacity * body + (1 - mesh_opacity) * bone.
  * The overlay restates cv2.addWeighted(color, 0.5, frame, 0.5, 0) as (c + o) / 2 rounded half to even; cv2 is not installed,
    so the overlay is UNVERIFIED against it.
  * The resize is bilinear with half-pixel centres, fp32 weights, round half to even; OpenCV's fixed-point INTER_LINEAR is NOT
    claimed bit for bit.
Refused by name: vis_traj, vis_cam, floor, shadows, the orthographic camera, vis_gtmesh, append_img, clean and gif / mp4 / jpg
writing.  Inference only."""
import numpy as np
import torch

from . import _lib as L
from . import abi
from .plasma_table import PLASMA

_C = abi.SEQVIS_CONSTANTS
STATUS_WORDS = _C["MODA_SEQVIS_STATUS_WORDS"]
DROPPED, NONFINITE, NAN_ERROR, EMPTY, BAD_INDEX = (_C["MODA_SEQVIS_" + k] for k in ("DROPPED", "NONFINITE", "NAN_ERROR", "EMPTY",
                                                                                  "BAD_INDEX"))
REC_FLOATS = _C["MODA_SEQVIS_REC_FLOATS"]
_REC_DOUBLES, _BOX_INTS = abi.CONSTANTS["MODA_RASTER_REC_DOUBLES"], abi.CONSTANTS["MODA_RASTER_BOX_INTS"]
BUDGET_BYTES = 1 << 30
MAX_VIEWS = 65535                      # views of one launch (the grid's second dimension)
GRAY_BASE = (3 * 128) // 5             # render_vis.py:152 then :335
_REFUSED = {
    "vis_traj": "vertex trajectories are GL line primitives, which the triangle rasteriser does not draw",
    "vis_cam": "camera glyphs in the scene are not implemented (moda_amd.cams.draw_cams builds the glyph mesh)",
    "floor": "the floor needs the reference's mesh_material/wood.obj",
    "shadows": "directional shadows are not implemented",
    "vis_gtmesh": "ground-truth meshes change topology from frame to frame: render them with mesh_render.render_mesh per frame",
    "append_img": "prepending the input frames is not implemented",
    "clean": "extract_mesh already keeps the largest connected part",
    "gif": "writing gif files is not implemented", "mp4": "writing mp4 files is not implemented",
    "jpg": "writing jpg files is not implemented", "outpath": "writing gif / mp4 / jpg files is not implemented",
}


class SeqRender:
    """What render_sequence returns, all device tensors: color (F, H, W, 3) uint8, depth (F, H, W) fp32, sil (F, H, W) int16 =
    100 * (depth > 0), frames (F, h, out_width, 3) uint8, refsil (F, h, out_width) int16, ctrajs (F, 4, 4) fp32 = [R | T] over the
    rendered camera's K row times out_width / W, cams (F, 4, 4) the cameras rendered with, and status, an int32 device word of
    STATUS_WORDS counts: [DROPPED] faces dropped behind the camera, [NONFINITE] non-finite projected vertices, [NAN_ERROR] NaN
    error values, [EMPTY] frames with an empty silhouette, [BAD_INDEX] faces indexing a vertex that does not exist."""

    def __init__(self, color, depth, sil, frames, refsil, ctrajs, cams, status):
        self.color, self.depth, self.sil, self.frames, self.refsil = color, depth, sil, frames, refsil
        self.ctrajs, self.cams, self.status = ctrajs, cams, status

    def __len__(self):
        return int(self.color.shape[0])

    def save_ctrajs(self, prefix):
        """The reference's `%s-ctrajs-%05d.txt` files (render_vis.py:531-533), np.savetxt of each 4 x 4.  The only read-back of
        this module.  -> the list of paths."""
        host = self.ctrajs.detach().cpu().numpy()
        paths = []
        for i in range(len(host)):
            paths.append('%s-ctrajs-%05d.txt' % (prefix, i))
            np.savetxt(paths[-1], host[i])
        return paths


def _refuse(options):
    for name, value in options.items():
        if name == "cam_type":
            if value != "perspective":
                raise NotImplementedError(f"render_sequence: cam_type = {value!r}: the orthographic camera is not implemented")
        elif name in _REFUSED:
            if value not in (None, False, "", "no", 0):
                raise NotImplementedError(f"render_sequence: {name}: {_REFUSED[name]}")
        else:
            raise TypeError(f"render_sequence: unknown option {name!r}")


def _device_tensor(what, t, dtype=None):
    if not torch.is_tensor(t):
        raise TypeError(f"render_sequence: {what} must be a tensor, got {type(t).__name__}")
    if t.requires_grad:
        raise NotImplementedError(f"render_sequence: {what} requires grad: mesh rendering is inference only and has no backward; "
                                  "pass it detached")
    if not t.is_cuda:
        raise RuntimeError(f"render_sequence: {what} is a CPU tensor; the HIP library is the only compute path")
    return t if dtype is None else L.dev(t, dtype)


def vertex_csr(faces, V):
    """The vertex -> (face, corner) incidence of a topology as a CSR: faces (Nf, 3) integer device tensor -> (offsets (V + 1),
    entries (3 Nf)) int32, entries 3 face + corner, those of vertex v at offsets[v] .. offsets[v + 1] in ascending order (a stable
    sort by vertex).  Corners that index no vertex of [0, V) are parked behind offsets[V].  No host read."""
    flat = faces.reshape(-1).long()
    key = torch.where((flat >= 0) & (flat < V), flat, torch.full_like(flat, V))
    skey, order = torch.sort(key, stable=True)
    offsets = torch.searchsorted(skey, torch.arange(V + 1, device=faces.device))
    return offsets.to(torch.int32).contiguous(), order.to(torch.int32).contiguous()


def _cached_csr(holder, slot, faces, V):
    """The CSR of `faces`, kept on `holder` (the sequence) per topology: rebuilt when the tensor or its version changes."""
    cache = getattr(holder, "_seqvis_csr", None) if holder is not None else None
    if cache is None:
        cache = {}
        if holder is not None:
            holder._seqvis_csr = cache
    hit = cache.get(slot)
    if hit is not None and hit[0] is faces and hit[1] == faces._version and hit[2] == V:
        return hit[3]
    csr = vertex_csr(faces, V)
    cache[slot] = (faces, faces._version, V, csr)
    return csr


def frames_per_chunk(budget_bytes, S, layers):
    """Frames of one chunk: `layers` = [(V, Nf), ...] of the raster passes.  Per frame: the per-view faces (12 Nf), the
    rasteriser's rec and box workspace (12 doubles + 4 ints per face), the camera-frame and NDC vertices and the records (56 V), and
    per layer the S x S planes face_idx, bary, zbuf and alpha (24 S S); held under the rasteriser's B S S < 2^31 and B Nf < 2^31
    and the launch's MAX_VIEWS.  At least 1."""
    per = sum(Nf * (12 + 8 * _REC_DOUBLES + 4 * _BOX_INTS) + V * (12 + 12 + 4 * REC_FLOATS) + 24 * S * S for V, Nf in layers)
    n = max(1, int(budget_bytes) // per)
    for V, Nf in layers:
        n = min(n, (2 ** 31 - 1) // (S * S), (2 ** 31 - 1) // (3 * max(Nf, V)), (2 ** 28 - 1) // V)
    return max(1, min(n, MAX_VIEWS))


class _Layer:
    """One raster pass: a topology, its CSR and the chunk-sized workspaces."""

    def __init__(self, verts, faces, colors, csr, n, S, dev):
        self.verts, self.faces, self.colors, self.csr = verts, faces, colors, csr
        self.V, self.Nf = int(verts.shape[1]), int(faces.shape[0])
        V, Nf = self.V, self.Nf
        self.cam = torch.empty((n, V, 3), device=dev)
        self.ndc = torch.empty((n, V, 3), device=dev)
        self.view_faces = torch.empty((n, Nf, 3), dtype=torch.int32, device=dev)
        self.rec = torch.empty((n, V, REC_FLOATS), device=dev)
        self.rast_rec = torch.empty((n * Nf, _REC_DOUBLES), dtype=torch.float64, device=dev)
        self.rast_box = torch.empty((n * Nf, _BOX_INTS), dtype=torch.int32, device=dev)
        self.face_idx = torch.empty((n, S, S), dtype=torch.int32, device=dev)
        self.bary = torch.empty((n, S, S, 3), device=dev)
        self.zbuf = torch.empty((n, S, S), device=dev)
        self.alpha = torch.empty((n, S, S), device=dev)

    def run(self, f0, n, cams, S, znear, zfar, mode, const, error, table, status):
        V, Nf = self.V, self.Nf
        Fv = int(self.verts.shape[0])
        verts = self.verts if Fv == 1 else self.verts[f0:f0 + n]
        L.call("moda_seqvis_project", L.ptr(verts), L.ptr(cams[f0:f0 + n]), L.ptr(self.faces), n, 1 if Fv == 1 else n, V, Nf, S,
               L.ptr(self.cam), L.ptr(self.ndc), L.ptr(self.view_faces), L.ptr(status), L.stream())
        colors, Fc = self.colors, 1
        if colors is not None and colors.dim() == 3:
            colors, Fc = colors[f0:f0 + n], n
        L.call("moda_seqvis_records", L.ptr(self.cam), L.ptr(self.view_faces), L.ptr(self.csr[0]), L.ptr(self.csr[1]), n, V, Nf, mode,
               L.ptr(colors), Fc, float(const), L.ptr(None if error is None else error[f0:f0 + n]), L.ptr(table), L.ptr(self.rec),
               L.ptr(status), L.stream())
        L.call("moda_raster_fwd", L.ptr(self.ndc), L.ptr(self.view_faces), 1, n, V, Nf, S, float(znear), float(zfar), 1,
               L.ptr(self.rast_rec), L.ptr(self.rast_box), L.ptr(self.face_idx), L.ptr(self.bary), L.ptr(self.zbuf), L.ptr(self.alpha),
               L.stream())


def shade(body, bone, n, S, H, W, smooth, opacity, overlay, color, depth, sil, sil_count):
    """moda_seqvis_shade on raster planes: body / bone = (face_idx (n,S,S), bary (n,S,S,3), zbuf (n,S,S), faces (Nf,3), rec
    (n,V,8), cam (n,V,3)) device tensors (bone None for one layer), written into color (n,H,W,3) uint8, depth (n,H,W), sil (n,H,W)
    int16; sil_count (n) int32 is added to."""
    args = []
    for layer in (body, bone):
        if layer is None:
            args += [None] * 6 + [0, 0]
        else:
            fi, ba, zb, fa, rec, cam = layer
            args += [L.ptr(t) for t in (fi, ba, zb, fa, rec, cam)] + [int(rec.shape[1]), int(fa.shape[0])]
    L.call("moda_seqvis_shade", *args, n, S, H, W, int(bool(smooth)), float(opacity), L.ptr(overlay), L.ptr(color), L.ptr(depth),
           L.ptr(sil), L.ptr(sil_count), L.stream())


def resize(color, sil, sil_count, h, w, status):
    """moda_seqvis_resize: color (n,H,W,3) uint8, sil (n,H,W) int16 -> (frames (n,h,w,3) uint8, refsil (n,h,w) int16)."""
    n, H, W = (int(s) for s in sil.shape)
    frames = torch.empty((n, h, w, 3), dtype=torch.uint8, device=color.device)
    refsil = torch.empty((n, h, w), dtype=torch.int16, device=color.device)
    L.call("moda_seqvis_resize", L.ptr(color), L.ptr(sil), L.ptr(sil_count), n, H, W, h, w, L.ptr(frames), L.ptr(refsil),
           L.ptr(status), L.stream())
    return frames, refsil


def view_cameras(rtk, verts, image_hw, vp=0, turntable=False, out_width=480):
    """Stage 1 alone: rtk (F,4,4), verts (F,V,3) or (1,V,3) device tensors -> (cams (F,4,4), ctrajs (F,4,4))."""
    H, W = (int(x) for x in image_hw)
    F = int(rtk.shape[0])
    cams = torch.empty((F, 4, 4), device=rtk.device)
    ctrajs = torch.empty((F, 4, 4), device=rtk.device)
    L.call("moda_seqvis_cams", L.ptr(rtk), L.ptr(verts), F, int(verts.shape[0]), int(verts.shape[1]), int(vp), int(bool(turntable)),
           W, H, int(out_width), L.ptr(cams), L.ptr(ctrajs), L.stream())
    return cams, ctrajs


@torch.no_grad()
def render_sequence(seq, image_hw, *, vp=0, freeze=False, rest=False, bones=False, mesh_opacity=254 / 255, smooth=True,
                    gray_color=False, vertex_error=None, overlay=None, out_width=480, cams=None, znear=1e-3, zfar=1000.0,
                    budget_bytes=BUDGET_BYTES, **options):
    """seq: a MeshSequence, or (verts (F,V,3), faces (Nf,3), colors (F,V,3)|(V,3) uint8, rtk (F,4,4)).  image_hw = (H, W) of the
    input frames; the render is square, S = max(H, W) (render_vis.py:262, 279), and cropped to H x W.
    vp: 0 the frame's camera, 1 / 2 a quarter turn about y / x re-centred on the frame's vertex mean, -1 the static first camera,
    -2 the canonical camera.  freeze / rest: the turntable over frame 0's / the rest vertices (and its bones).  bones: a second
    raster pass over seq.bone_mesh, composited with mesh_opacity (254 / 255: the reference's mark; 0.5 is the useful one).
    smooth: interpolated vertex normals, else face normals.  Colours: floor(0.6 colour); gray_color: 76; vertex_error (F,V):
    plasma(5 error), NaN -> (0, 0, 0) and counted.  overlay (F,H,W,3) uint8 RGB: the input frames, blended half and half.  cams
    (F,4,4) replaces seq.rtk (--root_frames).  -> SeqRender.  See the module docstring for what is restated and what departs."""
    _refuse(options)
    is_seq = not isinstance(seq, (tuple, list))
    if is_seq:
        verts, faces, colors, rtk = seq.verts, seq.faces, seq.colors, seq.rtk
    else:
        if len(seq) != 4:
            raise ValueError(f"render_sequence: seq must be a MeshSequence or (verts, faces, colors, rtk), got {len(seq)} items")
        verts, faces, colors, rtk = seq
    if cams is not None:
        rtk = cams
    if len(tuple(image_hw)) != 2 or min(int(x) for x in image_hw) < 1:
        raise ValueError(f"render_sequence: image_hw must be (H, W) >= 1, got {image_hw!r}")
    H, W = (int(x) for x in image_hw)
    S, ow = max(H, W), int(out_width)
    if ow < 1 or int(H * ow / W) < 1:
        raise ValueError(f"render_sequence: out_width = {out_width} gives an empty frame for image_hw = {(H, W)}")
    h = int(H * ow / W)                                                               # render_vis.py:212
    if S > 32768:
        raise ValueError(f"render_sequence: image_hw = {(H, W)}: the render size {S} exceeds 32768")
    if int(vp) not in (-2, -1, 0, 1, 2):
        raise ValueError(f"render_sequence: vp = {vp!r}, expected one of -2, -1, 0, 1, 2")
    if freeze and rest:
        raise ValueError("render_sequence: freeze and rest are two turntables; choose one")
    if not 0.0 <= float(mesh_opacity) <= 1.0:
        raise ValueError(f"render_sequence: mesh_opacity = {mesh_opacity} outside [0, 1]")
    verts = _device_tensor("verts", verts, torch.float32)
    faces = _device_tensor("faces", faces, torch.int32)
    rtk = _device_tensor("cams" if cams is not None else "rtk", rtk, torch.float32)
    if verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[0] < 1 or verts.shape[1] < 1:
        raise ValueError(f"render_sequence: verts must be (F, V, 3) with F, V >= 1, got {tuple(verts.shape)}")
    F, V = int(verts.shape[0]), int(verts.shape[1])
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError(f"render_sequence: faces must be (Nf, 3) with Nf >= 1, got {tuple(faces.shape)}")
    if tuple(rtk.shape) != (F, 4, 4):
        raise ValueError(f"render_sequence: {'cams' if cams is not None else 'rtk'} must be ({F}, 4, 4), got {tuple(rtk.shape)}")
    dev = verts.device
    turntable = bool(freeze or rest)
    if rest and (not is_seq or getattr(seq, "rest_verts", None) is None):
        raise ValueError("render_sequence: rest needs a MeshSequence with rest_verts")
    if bones and (not is_seq or getattr(seq, "bone_mesh", None) is None):
        raise ValueError("render_sequence: bones needs a MeshSequence with bone_mesh")
    # the vertices and colours every view draws
    if rest:
        body_verts = _device_tensor("rest_verts", seq.rest_verts, torch.float32)[None]
        if tuple(body_verts.shape) != (1, V, 3):
            raise ValueError(f"render_sequence: rest_verts must be ({V}, 3), got {tuple(seq.rest_verts.shape)}")
        if getattr(seq, "rest_colors", None) is not None:
            colors = seq.rest_colors
    else:
        body_verts = verts[:1] if freeze else verts
    mode, const, error, table = _C["MODA_SEQVIS_COLOR_U8"], 0.0, None, None
    if vertex_error is not None:
        if turntable:
            raise ValueError("render_sequence: vertex_error colours frames; it cannot be combined with freeze / rest")
        error = _device_tensor("vertex_error", vertex_error, torch.float32)
        if tuple(error.shape) != (F, V):
            raise ValueError(f"render_sequence: vertex_error must be ({F}, {V}), got {tuple(error.shape)}")
        mode, colors = _C["MODA_SEQVIS_COLOR_ERROR"], None
        table = L.const_tensor("seqvis_plasma", dev, lambda: np.asarray(PLASMA, np.float32))
    elif gray_color:
        mode, const, colors = _C["MODA_SEQVIS_COLOR_CONST"], float(GRAY_BASE), None
    else:
        colors = _device_tensor("colors", colors, torch.uint8)
        if colors.dim() not in (2, 3) or tuple(colors.shape[-2:]) != (V, 3) or (colors.dim() == 3 and colors.shape[0] != F):
            raise ValueError(f"render_sequence: colors must be ({F}, {V}, 3) or ({V}, 3) uint8, got {tuple(colors.shape)}")
        if colors.dim() == 3 and (freeze or F == 1):
            colors = colors[0]
    if overlay is not None:
        overlay = _device_tensor("overlay", overlay)
        if overlay.dtype != torch.uint8 or tuple(overlay.shape) != (F, H, W, 3):
            raise ValueError(f"render_sequence: overlay must be ({F}, {H}, {W}, 3) uint8, got {tuple(overlay.shape)} {overlay.dtype}")
        overlay = overlay.contiguous()
    bone = None
    if bones:
        bv, bf, bc = seq.bone_rest_mesh if rest else seq.bone_mesh
        bv, bf, bc = (_device_tensor("bone_mesh", bv, torch.float32), _device_tensor("bone_mesh", bf, torch.int32),
                      _device_tensor("bone_mesh", bc, torch.uint8))
        if bv.dim() != 3 or bv.shape[2] != 3 or bv.shape[0] not in (1, F) or tuple(bf.shape[1:]) != (3,) or tuple(bc.shape) != (bv.shape[1], 3):
            raise ValueError(f"render_sequence: bone_mesh must be (verts (F, Vb, 3), faces (Nb, 3), colors (Vb, 3)), got "
                             f"{tuple(bv.shape)}, {tuple(bf.shape)}, {tuple(bc.shape)}")
        if turntable or bv.shape[0] == 1:
            bv = bv[:1]                                                               # tbone = 0 (:428-431)
        bone = (bv, bf, bc)

    status = torch.zeros(STATUS_WORDS, dtype=torch.int32, device=dev)
    view_cams, ctrajs = view_cameras(rtk, body_verts, (H, W), vp, turntable, ow)
    sizes = [(V, int(faces.shape[0]))] + ([(int(bone[0].shape[1]), int(bone[1].shape[0]))] if bone else [])
    per = min(F, frames_per_chunk(budget_bytes, S, sizes))
    holder = seq if is_seq else None
    body_layer = _Layer(body_verts, faces, colors, _cached_csr(holder, "body", faces, V), per, S, dev)
    bone_layer = None
    if bone:
        bone_layer = _Layer(bone[0], bone[1], bone[2], _cached_csr(holder, "bone", bone[1], int(bone[0].shape[1])), per, S, dev)
    color = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((F, H, W), device=dev)
    sil = torch.empty((F, H, W), dtype=torch.int16, device=dev)
    frames = torch.empty((F, h, ow, 3), dtype=torch.uint8, device=dev)
    refsil = torch.empty((F, h, ow), dtype=torch.int16, device=dev)
    sil_count = torch.zeros(F, dtype=torch.int32, device=dev)
    planes = lambda l: (l.face_idx, l.bary, l.zbuf, l.faces, l.rec, l.cam)
    for f0 in range(0, F, per):
        n = min(per, F - f0)
        body_layer.run(f0, n, view_cams, S, znear, zfar, mode, const, error, table, status)
        if bone_layer:
            bone_layer.run(f0, n, view_cams, S, znear, zfar, _C["MODA_SEQVIS_COLOR_U8"], 0.0, None, None, status)
        shade(planes(body_layer), planes(bone_layer) if bone_layer else None, n, S, H, W, smooth, mesh_opacity,
              None if overlay is None else overlay[f0:f0 + n], color[f0:f0 + n], depth[f0:f0 + n], sil[f0:f0 + n],
              sil_count[f0:f0 + n])
        L.call("moda_seqvis_resize", L.ptr(color[f0:f0 + n]), L.ptr(sil[f0:f0 + n]), L.ptr(sil_count[f0:f0 + n]), n, H, W, h, ow,
               L.ptr(frames[f0:f0 + n]), L.ptr(refsil[f0:f0 + n]), L.ptr(status), L.stream())
    return SeqRender(color, depth, sil, frames, refsil, ctrajs, view_cams, status)
