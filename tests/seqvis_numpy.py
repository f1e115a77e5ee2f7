"""Float64 numpy restatement of every stage of moda_amd/seq_render.py (include/moda_hip_seqvis.h), itself a restatement of
scripts/visualize/render_vis.py:246-511.  Imports nothing from the package.  The reference script cannot run here (pyrender,
trimesh and cv2 are absent), so the viewpoint block, the compositing, the overlay and the resize are RESTATED AND UNPINNED; what is
pinned from outside (tests/test_seqvis_oracle.py): `rodrigues` to scipy, `plasma_lookup` to matplotlib, `obj_to_cam` / `pixels` to
oracle/torch_ref.py.  Inputs are taken as given (fp32 arrays are widened, never re-rounded).  U = 2^-24, the fp32 unit round-off.

Running fp32 bounds (first order, every fp32 operation rounding once = U relative, contraction off):
  obj_to_cam   X = ((r0 x + r1 y) + r2 z) + t: three products and three sums, each partial result at most the sum of the
               magnitudes M = |r0 x| + |r1 y| + |r2 z| + |t|:  E_X = 4 U M  (a term passes through at most 4 roundings).
  pixels       u = fx X / Zs + px: E_u = |fx| E_X / |Zs| + |fx X| E_Z / Zs^2 + 2 U |fx X / Zs| + U |u|
               (the product fx X and the division round once each, then the sum).
  ndc          x = u sc - 1, sc = fp32(2 / S): E = |sc| E_u + 2 U |u sc| + U |x|  (sc's own rounding, the product, the sum).
  normals      a cross-product component ab - cd of differences: each difference rounds once, each product once, the
               difference of products once: 4 U (|ab| + |cd|) covers them; k faces added one at a time add (k - 1) U times the
               sum of the magnitudes.  n / max(|n|, 1e-12): |n| carries (E_n . n) / |n| + 3 U |n| (two sums, a square root that
               halves what it is given, three squares), the quotient one more U."""
import numpy as np

U = 2.0 ** -24
STATUS = {"dropped": 0, "nonfinite": 1, "nan_error": 2, "empty": 3, "bad_index": 4}


# ---- stage 1 ----------------------------------------------------------------------------------------------------------------------
def rodrigues(r):
    """cv2.Rodrigues of a rotation vector by its published formula: cos I + (1 - cos) k k^T + sin [k]x, k = r / |r|; I at 0."""
    r = np.asarray(r, np.float64)
    th = np.sqrt(r.dot(r))
    if th == 0.0:
        return np.eye(3)
    k = r / th
    c, s = np.cos(th), np.sin(th)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return c * np.eye(3) + (1 - c) * np.outer(k, k) + s * kx


def view_cameras(rtk, verts, image_hw, vp=0, turntable=False, out_width=480):
    """render_vis.py:259-322 -> (cams (F,4,4), ctrajs (F,4,4)) float64.  verts (F,V,3) or (1,V,3).  ctrajs' K row is the fp32
    rounding of the camera's K row times out_width / W."""
    rtk = np.asarray(rtk, np.float64)
    verts = np.asarray(verts, np.float64)
    H, W = image_hw
    F = len(rtk)
    cams, ctrajs = np.zeros((F, 4, 4)), np.zeros((F, 4, 4))
    for i in range(F):
        cam0 = rtk[0]
        refcam = rtk[i].copy()
        if turntable:
            refcam = cam0.copy()
            refcam[:3, :3] = rodrigues([0., i * 2 * np.pi / F, 0.]).dot(refcam[:3, :3])
            refcam[:2, 3] = 0
            refcam[3, 2], refcam[3, 3] = W / 2, H / 2
        v = verts[0 if len(verts) == 1 else i]
        vp_tmat, vp_kmat = refcam[:3, 3].copy(), refcam[3].copy()
        if vp == -1:
            vp_rmat = cam0[:3, :3].dot(refcam[:3, :3].T)
            vp_tmat = cam0[:3, 3].copy()
            vp_kmat = cam0[3].copy()
            vp_kmat[2] = vp_kmat[2] / W * W
            vp_kmat[3] = vp_kmat[3] / H * H
        elif vp == -2:
            can = rodrigues([0, np.pi / 3, 0]).dot(rodrigues([np.pi, 0, 0]))
            vp_rmat = can.dot(refcam[:3, :3].T)
            vp_tmat = np.zeros(3)
            vp_tmat[2] = cam0[2, 3]
            vp_kmat = cam0[3].copy()
            vp_kmat[2] = vp_kmat[2] / W * W
            vp_kmat[3] = vp_kmat[3] / H * H
        elif vp == 1:
            vp_rmat = rodrigues([0, np.pi / 2, 0])
        elif vp == 2:
            vp_rmat = rodrigues([np.pi / 2, 0, 0])
        else:
            vp_rmat = rodrigues([0., 0, 0])
        out = refcam.copy()
        out[:3, :3] = vp_rmat.dot(refcam[:3, :3])
        if vp in (1, 2):
            vp_tmat[:2] = (-out[:3, :3].dot(v.mean(0)))[:2]
        out[:3, 3], out[3] = vp_tmat, vp_kmat
        cams[i] = out
        ctrajs[i] = out
        ctrajs[i, 3] = out[3].astype(np.float32).astype(np.float64) * (out_width / W)
    return cams, ctrajs


def ulp_diff(got32, want64, floor=1e-14):
    """|got - fp32(want)| in units of the fp32 spacing at the larger of the two.  A difference of at most `floor` counts as 0:
    an entry such as (C R^T R)[i, j] where C[i, j] = 0 is what cancellation leaves of terms of size 1, about 1e-16 in ANY float64
    evaluation and in no two the same, so the fp32 spacing AT that value (1e-23) measures nothing; 1e-14 is a hundred float64
    roundings of a term of size 1, and nine orders below the fp32 spacing of the entries that are not such residue."""
    got = np.asarray(got32, np.float32)
    want = np.asarray(want64, np.float64).astype(np.float32)
    gap = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return np.where(d <= floor, 0.0, d / gap.astype(np.float64))


# ---- stage 2 ----------------------------------------------------------------------------------------------------------------------
def obj_to_cam(verts, cam):
    v = np.asarray(verts, np.float64)
    c = np.asarray(cam, np.float64)
    return v.dot(c[:3, :3].T) + c[:3, 3]


def pixels(xyz, krow):
    """u = fx X / Zs + px, v = fy Y / Zs + py with Zs = Z, or 1e-12 within 1e-12 of 0 (fp32's 1e-12, as the device's)."""
    z = xyz[:, 2]
    zs = np.where(np.abs(z) < np.float64(np.float32(1e-12)), np.float64(np.float32(1e-12)), z)
    return krow[0] * xyz[:, 0] / zs + krow[2], krow[1] * xyz[:, 1] / zs + krow[3], zs


def _z32(verts, cam):
    """The fp32 camera Z as the device forms it, operation by operation: what decides Z > 0."""
    v, c = np.asarray(verts, np.float32), np.asarray(cam, np.float32)
    return ((c[2, 0] * v[:, 0] + c[2, 1] * v[:, 1]) + c[2, 2] * v[:, 2]) + c[2, 3]


def project(verts, cam, faces, S):
    """One view -> dict: cam (V,3), ndc (V,3) float64, their fp32 bounds cam_bound / ndc_bound, view_faces (Nf,3) (a dropped or
    out-of-range face (-1,-1,-1)), dropped / bad_index (Nf) bool.  The drop decision reads the fp32 Z (`_z32`): a sign is not
    a matter of tolerance."""
    v, c = np.asarray(verts, np.float64), np.asarray(cam, np.float64)
    faces = np.asarray(faces, np.int64)
    V = len(v)
    xyz = obj_to_cam(v, c)
    M = np.abs(v[:, None, :] * c[None, :3, :3]).sum(-1) + np.abs(c[:3, 3])[None]
    e_cam = 4 * U * M
    with np.errstate(all="ignore"):
        u, w, zs = pixels(xyz, c[3])
        sc = np.float64(np.float32(2.0 / S))
        ndc = np.stack([u * sc - 1.0, -(w * sc - 1.0), xyz[:, 2]], -1)
        bound = np.zeros_like(ndc)
        for a, (pix, f) in enumerate(((u, c[3, 0]), (w, c[3, 1]))):
            q = np.abs(f * xyz[:, a] / zs)
            e_pix = np.abs(f) * e_cam[:, a] / np.abs(zs) + np.abs(f * xyz[:, a]) * e_cam[:, 2] / zs ** 2 + 2 * U * q + U * np.abs(pix)
            bound[:, a] = sc * e_pix + 2 * U * np.abs(pix * sc) + U * np.abs(ndc[:, a])
        bound[:, 2] = e_cam[:, 2]
    in_range = ((faces >= 0) & (faces < V)).all(-1)
    z32 = _z32(verts, cam)
    front = np.zeros(len(faces), bool)
    front[in_range] = (z32[faces[in_range]] > 0).all(-1)
    keep = in_range & front
    vf = np.where(keep[:, None], faces, -1)
    return {"cam": xyz, "ndc": ndc, "cam_bound": e_cam, "ndc_bound": bound, "view_faces": vf, "dropped": in_range & ~front,
            "bad_index": ~in_range, "nonfinite": int((~np.isfinite(ndc).all(-1)).sum()), "z32": z32}


def vertex_csr(faces, V):
    """(offsets (V+1), entries): entry 3 face + corner, a vertex's entries ascending; out-of-range corners behind offsets[V]."""
    flat = np.asarray(faces, np.int64).reshape(-1)
    key = np.where((flat >= 0) & (flat < V), flat, V)
    order = np.argsort(key, kind="stable")
    return np.searchsorted(key[order], np.arange(V + 1)), order


def vertex_normals(cam, view_faces):
    """Area-weighted unit vertex normals of one view -> (normals (V,3) float64, bound (V,3)): see the module docstring."""
    p = np.asarray(cam, np.float64)
    V = len(p)
    n, e, mag, cnt = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V)
    for f in np.asarray(view_faces, np.int64):
        if f[0] < 0:
            continue
        a, b = p[f[1]] - p[f[0]], p[f[2]] - p[f[0]]
        fn = np.cross(a, b)
        fe = 4 * U * np.array([abs(a[1] * b[2]) + abs(a[2] * b[1]), abs(a[2] * b[0]) + abs(a[0] * b[2]), abs(a[0] * b[1]) + abs(a[1] * b[0])])
        for k in f:
            n[k] += fn
            e[k] += fe
            mag[k] += np.abs(fn)
            cnt[k] += 1
    e += np.maximum(cnt - 1, 0)[:, None] * U * mag
    length = np.sqrt((n * n).sum(-1))
    safe = np.maximum(length, 1e-12)
    unit = n / safe[:, None]
    e_len = (e * np.abs(n)).sum(-1) / safe + 3 * U * length
    bound = e / safe[:, None] + np.abs(unit) * (e_len / safe)[:, None] + U * np.abs(unit)
    return unit, bound


# ---- stage 3 ----------------------------------------------------------------------------------------------------------------------
def base_u8(colors):
    """floor(0.6 c) (render_vis.py:335, through uint8)."""
    return np.floor(0.6 * np.asarray(colors, np.uint8).astype(np.float64))


def plasma_lookup(x, table):
    """matplotlib's Colormap.__call__ for float input on a 256-entry table (256,3): index int(x 256); x < 0 the first entry,
    x >= 1 the last, NaN the bad colour (0, 0, 0).  x is taken in fp32, as the reference hands matplotlib fp32 distances.
    -> (rgb (...,3), nan mask)."""
    x = np.asarray(x, np.float32)
    table = np.asarray(table)
    nan = np.isnan(x)
    xa = np.where(nan, 0, x).astype(np.float64) * 256
    idx = np.where(xa < 0, 0, np.where(xa >= 256, 255, np.minimum(xa, 255).astype(np.int64)))
    out = table[idx].astype(np.float64)
    out[nan] = 0
    return out, nan


def error_colors(err, table):
    x = np.float32(5.0) * np.asarray(err, np.float32)
    return plasma_lookup(x, table)


# ---- stage 4 ----------------------------------------------------------------------------------------------------------------------
def _layer(face_idx, bary, zbuf, faces, rec, cam, smooth):
    """-> (on (H,W), rgb (H,W,3) float64 clamped, z, edge: a channel within 1e-4 of the clamp at 255)."""
    faces = np.asarray(faces, np.int64)
    rec, cam = np.asarray(rec, np.float64), np.asarray(cam, np.float64)
    fi = np.asarray(face_idx, np.int64)
    on = (fi >= 0) & (fi < len(faces))
    f = faces[np.where(on, fi, 0)]
    on &= ((f >= 0) & (f < len(rec))).all(-1)
    f = np.where(on[..., None], f, 0)
    b = np.asarray(bary, np.float64)
    r = rec[f]                                                                        # (H,W,3,8)
    rgb = (b[..., None] * r[..., :3]).sum(-2)
    if smooth:
        n = (b[..., None] * r[..., 3:6]).sum(-2)
    else:
        p = cam[f]
        n = np.cross(p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :])
    lam = np.abs(n[..., 2]) / np.maximum(np.sqrt((n * n).sum(-1)), 1e-12)
    pre = rgb * (0.4 + lam)[..., None]
    rgb = np.clip(pre, 0.0, 255.0)
    edge = on & (np.abs(pre - 255.0) < 1e-4).any(-1)                                  # the clamp is a decision too
    return on, np.where(on[..., None], rgb, 0.0), np.where(on, np.asarray(zbuf, np.float64), 0.0), edge


def shade(body, bone, H, W, smooth=True, opacity=254 / 255, overlay=None, tol=1e-4):
    """One frame.  body / bone = (face_idx (S,S), bary (S,S,3), zbuf (S,S), faces, rec (V,8), cam (V,3)), bone None for one layer.
    opacity is taken in fp32, as the device receives it.  -> dict color (H,W,3) uint8, depth (H,W), sil (H,W) int16, near (H,W)
    bool: pixels a channel of which lies within `tol` of an integer before truncation, or of the clamp (a decision boundary)."""
    crop = lambda t: np.asarray(t)[:H, :W]
    on, rgb, z, edge = _layer(crop(body[0]), crop(body[1]), crop(body[2]), body[3], body[4], body[5], smooth)
    if bone is not None:
        onb, rgbb, zb, edgeb = _layer(crop(bone[0]), crop(bone[1]), crop(bone[2]), bone[3], bone[4], bone[5], smooth)
        op = np.float64(np.float32(opacity))
        both = on & onb
        front = both & (zb < z)
        mix = op * rgb + (np.float64(np.float32(1.0) - np.float32(opacity))) * rgbb
        out = np.where(both[..., None], np.where(front[..., None], rgbb, mix), np.where(on[..., None], rgb, rgbb))
        depth = np.where(both, np.minimum(z, zb), np.where(on, z, zb))
        edge = edge | edgeb
    else:
        out, depth = rgb, z
    # 0 and 255 exactly are what an absent layer and the clamp give on the device too: not boundaries (the clamp's own is `edge`)
    near = ((np.abs(out - np.round(out)) < tol) & (out != 0.0) & (out != 255.0)).any(-1) | edge
    c = np.floor(out).astype(np.int64)
    if overlay is not None:
        s = c + np.asarray(overlay, np.int64)
        c = s // 2
        c += (s & 1) * (c & 1)
    c = np.clip(c, 0, 255)
    c[0, 0] = 0
    near[0, 0] = False
    return {"color": c.astype(np.uint8), "depth": depth, "sil": (100 * (depth > 0)).astype(np.int16), "near": near}


# ---- stage 5 ----------------------------------------------------------------------------------------------------------------------
def _taps(d, src, dst):
    scale = np.float32(np.float64(src) / np.float64(dst))
    s = (np.arange(d, dtype=np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
    fl = np.floor(s)
    w1 = (s - fl).astype(np.float32)
    a = fl.astype(np.int64)
    return np.clip(a, 0, src - 1), np.clip(a + 1, 0, src - 1), w1


def resize(img, h, w, tol=1e-4):
    """Bilinear, half-pixel centres, fp32 weights (formed as the device forms them), float64 sums, round half to even.
    img (H,W) or (H,W,C) integers -> (out of img's dtype, near: within `tol` of a rounding boundary x.5)."""
    a = np.asarray(img)
    H, W = a.shape[:2]
    y0, y1, wy = _taps(h, H, h)
    x0, x1, wx = _taps(w, W, w)
    one = np.float32(1.0)
    w00 = ((one - wy)[:, None] * (one - wx)[None]).astype(np.float64)
    w01 = ((one - wy)[:, None] * wx[None]).astype(np.float64)
    w10 = (wy[:, None] * (one - wx)[None]).astype(np.float64)
    w11 = (wy[:, None] * wx[None]).astype(np.float64)
    f = a.astype(np.float64).reshape(H, W, -1)
    g = lambda yy, xx: f[yy][:, xx]
    v = w00[..., None] * g(y0, x0) + w01[..., None] * g(y0, x1) + w10[..., None] * g(y1, x0) + w11[..., None] * g(y1, x1)
    near = (np.abs(v - np.floor(v) - 0.5) < tol).any(-1)
    out = np.rint(v)
    if a.dtype == np.uint8:
        out = np.clip(out, 0, 255)
    return out.astype(a.dtype).reshape((h, w) + a.shape[2:]), near


# ---- the chain's comparison with render_mesh --------------------------------------------------------------------------------------
def edge_band(ndc, view_faces, S, H, W, tol=1e-3):
    """Pixels of the H x W window whose centre lies within `tol` px of a projected edge of a kept face (in pixel units:
    u = (x + 1) S / 2, v = (1 - y) S / 2) -> (H,W) bool."""
    ndc = np.asarray(ndc, np.float64)
    u, v = (ndc[:, 0] + 1) * S / 2, (1 - ndc[:, 1]) * S / 2
    cy, cx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    band = np.zeros((H, W), bool)
    for f in np.asarray(view_faces, np.int64):
        if f[0] < 0:
            continue
        for a, b in ((0, 1), (1, 2), (2, 0)):
            ax, ay, bx, by = u[f[a]], v[f[a]], u[f[b]], v[f[b]]
            dx, dy = bx - ax, by - ay
            L2 = dx * dx + dy * dy
            t = np.clip(((cx - ax) * dx + (cy - ay) * dy) / L2, 0, 1) if L2 > 0 else np.zeros_like(cx)
            band |= np.hypot(cx - (ax + t * dx), cy - (ay + t * dy)) < tol
    return band


# ---- shared builders of the tests --------------------------------------------------------------------------------------------------
def icosphere(subdiv=1):
    """(verts (V,3) float64, faces (Nf,3) int64): an icosahedron subdivided `subdiv` times (12 vertices of valence 5, the rest 6)."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v), np.asarray(f, np.int64)


def fan(valence=70):
    """A hub (vertex 0) with `valence` triangles around it, slightly coned -> (verts (valence + 1, 3), faces (valence, 3))."""
    a = 2 * np.pi * np.arange(valence) / valence
    rim = np.stack([np.cos(a), np.sin(a), 0.2 * np.cos(3 * a)], -1)
    verts = np.concatenate([[[0, 0, 0.3]], rim], 0)
    faces = np.stack([np.zeros(valence, np.int64), 1 + np.arange(valence), 1 + (np.arange(valence) + 1) % valence], -1)
    return verts, faces


def camera(R=None, t=(0, 0, 3.0), k=(40.0, 40.0, 24.0, 24.0)):
    c = np.eye(4)
    if R is not None:
        c[:3, :3] = R
    c[:3, 3], c[3] = t, k
    return c.astype(np.float32)
