"""float64 numpy restatement of the reference's rasteriser kernel (third_party/softras/soft_renderer/cuda/
soft_rasterize_cuda_kernel.cu) in the configuration MoDA uses (nnutils/moda.py:469-471: dist_func 'euclidean', sigma_val 1e-12,
aggr_func_rgb 'hard', aggr_func_alpha 'prod', texture_type 'vertex', fill_back = double_side True, near 1, far 100): the oracle
of tests/test_raster_oracle.py and tests/test_gpu_mesh_render.py.

One loop over the faces in index order, every pixel of a face's bounding box at once, no tiles, no lists: not the algorithm of
moda_amd/csrc/raster_kernels.hip.  Two stated departures from the kernel source, both also made by the HIP kernels:
  * alpha is the hard cover mask.  With sigma_val = 1e-12 the 'prod' aggregate 1 - prod(1 - sigmoid(sign d^2 / sigma)) is 1
    where a face covers the pixel centre and 0 elsewhere except within sqrt(dist_eps * sigma) = 3e-6 NDC of an edge (:352, :375,
    :399-403, :415-416, :465); those pixels are inside the edge margin this module reports.
  * a face whose determinant (:278-281) is exactly 0 is skipped: the clamp at +-1e-10 (:282) leaves its barycentrics without
    meaning, and it cannot colour a pixel (w_clip sums to < 1e-5 or zp is out of range).
Besides the image it returns, per pixel, the EDGE MARGIN min_k min(|w_k|, |1 - w_k|) over the faces whose bounding box holds the
pixel (check_border, :33-38) and the DEPTH MARGIN, the relative gap between the two nearest zp that pass the near / far test:
where both are large, an fp32 evaluation of the same rule must pick the same face."""
from collections import namedtuple

import numpy as np

Raster = namedtuple("Raster", "face_idx bary zbuf alpha edge_margin depth_margin")
DIST_EPS = np.log(1.0 / 1e-4 - 1.0)            # functional/soft_rasterize.py:35 with dist_eps = 1e-4


def pixel_centres(S):
    """(xp over columns, yp over image rows): :343-346, rows flipped."""
    i = np.arange(S, dtype=np.float64)
    return (2.0 * i + 1.0 - S) / S, (2.0 * (S - 1 - i) + 1.0 - S) / S


def rasterize(face_vertices, S, near=1.0, far=100.0, sigma_val=1e-12):
    """face_vertices (F,3,3): corner k of face f = (x, y, z).  -> Raster of (S,S) arrays (bary (S,S,3))."""
    fv = np.asarray(face_vertices, np.float64).reshape(-1, 3, 3)
    xs, ys = pixel_centres(S)
    thr = np.sqrt(DIST_EPS * sigma_val)                                       # :352, :375
    face_idx = np.full((S, S), -1, np.int64)
    bary = np.zeros((S, S, 3))
    zbest = np.full((S, S), 10000000.0)                                       # :367
    zsecond = np.full((S, S), np.inf)
    alpha = np.zeros((S, S), bool)
    margin = np.full((S, S), np.inf)
    for fn, face in enumerate(fv):
        p = face[:, :2]
        det = p[2, 0] * (p[0, 1] - p[1, 1]) + p[0, 0] * (p[1, 1] - p[2, 1]) + p[1, 0] * (p[2, 1] - p[0, 1])     # :278-281
        if det == 0 or not np.isfinite(det):
            continue
        star = np.array([[p[1, 1] - p[2, 1], p[2, 0] - p[1, 0], p[1, 0] * p[2, 1] - p[2, 0] * p[1, 1]],
                         [p[2, 1] - p[0, 1], p[0, 0] - p[2, 0], p[2, 0] * p[0, 1] - p[0, 0] * p[2, 1]],
                         [p[0, 1] - p[1, 1], p[1, 0] - p[0, 0], p[0, 0] * p[1, 1] - p[1, 0] * p[0, 1]]])         # :274-277
        inv = star / (max(det, 1e-10) if det > 0 else min(det, -1e-10))      # :282-286
        # check_border (:33-38, :375): the pixels the reference does not skip
        cols = np.nonzero(~((xs > p[:, 0].max() + thr) | (xs < p[:, 0].min() - thr)))[0]
        rows = np.nonzero(~((ys > p[:, 1].max() + thr) | (ys < p[:, 1].min() - thr)))[0]
        if len(cols) == 0 or len(rows) == 0:
            continue
        sl = (slice(rows[0], rows[-1] + 1), slice(cols[0], cols[-1] + 1))
        X, Y = xs[sl[1]][None, :], ys[sl[0]][:, None]
        w = inv[:, 0, None, None] * X + inv[:, 1, None, None] * Y + inv[:, 2, None, None]        # (3, r, c)  :25-29
        margin[sl] = np.minimum(margin[sl], np.minimum(np.abs(w), np.abs(1.0 - w)).min(0))
        inside = ((w <= 1) & (w >= 0)).all(0)                                 # :47-50
        if not inside.any():
            continue
        alpha[sl] |= inside                                                   # before the depth range test (:408-424)
        wc = np.clip(w, 0.0, 1.0)                                             # :53-58
        wc = wc / np.maximum(wc.sum(0), 1e-5)
        with np.errstate(divide="ignore", invalid="ignore"):
            zp = 1.0 / (wc[0] / face[0, 2] + wc[1] / face[1, 2] + wc[2] / face[2, 2])            # :423
        ok = inside & ~((zp < near) | (zp > far))                             # :424 (a NaN zp passes here and loses below)
        zb, z2 = zbest[sl], zsecond[sl]
        better = ok & (zp < zb)                                               # :429: strict, in face order; both windings
        z2 = np.where(better, np.where(zb < 10000000.0, zb, z2), np.where(ok & (zp < z2), zp, z2))
        zsecond[sl] = z2
        zbest[sl] = np.where(better, zp, zb)
        face_idx[sl] = np.where(better, fn, face_idx[sl])
        bary[sl] = np.where(better[..., None], np.moveaxis(wc, 0, -1), bary[sl])
    hit = face_idx >= 0
    zbuf = np.where(hit, zbest, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        depth_margin = np.where(hit, (zsecond - zbest) / np.abs(zbest), np.inf)
    return Raster(face_idx, bary, zbuf, alpha, margin, depth_margin)


def interpolate(face_attrs, r, background=0.0):
    """face_attrs (F,3,C): corner k of face f.  -> (C,S,S): sum_k w_clip_k attr_k (:190-191), background where nothing won."""
    fa = np.asarray(face_attrs, np.float64)
    C = fa.shape[-1]
    bg = np.broadcast_to(np.asarray(background, np.float64), (C,))
    hit = r.face_idx >= 0
    a = fa[np.where(hit, r.face_idx, 0)]                                      # (S,S,3,C)
    img = (r.bary[..., None] * a).sum(2)
    return np.moveaxis(np.where(hit[..., None], img, bg), -1, 0)


def render(face_vertices, face_textures, S, background=(0.0, 0.0, 0.0), near=1.0, far=100.0, sigma_val=1e-12):
    """One view as the reference returns it: (C + 1, S, S) = colour channels + alpha, and the Raster."""
    r = rasterize(face_vertices, S, near, far, sigma_val)
    img = interpolate(face_textures, r, background)
    return np.concatenate([img, r.alpha[None].astype(np.float64)], 0), r


def forward_soft_rasterize(face_vertices, textures, faces_info, aggrs_info, soft_colors, image_size, near, far, eps, sigma_val,
                           func_dist_type, dist_eps, gamma_val, func_rgb_type, func_alpha_type, texture_type, fill_back):
    """Stand-in for soft_renderer.cuda.soft_rasterize.forward_soft_rasterize with the reference's argument list
    (functional/soft_rasterize.py:55-62), for torch CPU tensors; only MoDA's configuration."""
    import torch
    assert (func_dist_type, func_rgb_type, func_alpha_type, texture_type) == (2, 0, 2, 1) and fill_back
    fv, tex = face_vertices.detach().cpu().numpy(), textures.detach().cpu().numpy()
    bg = soft_colors.detach().cpu().numpy().astype(np.float64)
    for b in range(fv.shape[0]):
        img, r = render(fv[b], tex[b], image_size, near=near, far=far, sigma_val=sigma_val)
        hit = r.face_idx >= 0
        bg[b, :3] = np.where(hit[None], img[:3], bg[b, :3])                   # :468-472: written only where a face won
        bg[b, 3] = img[3]
        aggrs_info[b, 0] = torch.as_tensor(np.where(hit, r.zbuf, 10000000.0))
        aggrs_info[b, 1] = torch.as_tensor(r.face_idx.astype(np.float64))
    return faces_info, aggrs_info, torch.as_tensor(bg).to(soft_colors.dtype)


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions, radius=1.0):
    """-> (vertices (V,3) float64, faces (F,3) int64): 20 * 4^subdivisions faces, outward winding."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v) * radius, np.asarray(f, np.int64)


def views(v, seeds, shift=(0.0, 0.0, 3.0), scale=1.0):
    """(len(seeds), V, 3) fp32: the vertices under the rotation of each seed, scaled, then shifted (depth 3 by default)."""
    return np.stack([v @ rotation(s).T * scale + np.asarray(shift) for s in seeds]).astype(np.float32)


def sphere_volume(n=32):
    """The synthetic SDF of tests/test_gpu_marching_cubes.py (`sphere`: off-lattice centre, radius 0.35 n), restated."""
    ax = [np.arange(n, dtype=np.float64) - (n - 1) / 2 + o for o in (0.137, 0.071, -0.053)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return (0.35 * n - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)


def replicas(f):
    """Face lists that hold every face of f (F,3) more than once, as (name, faces, index of the lowest copy of face i).
    Copies have identical records, so they tie in depth at every pixel and the lowest copy must win: the image is the one of
    f alone with face i renamed.  Where the copies sit decides which ordering they test: `tile` puts them F apart (other
    256-face chunks, other flushes of the waiting list), `mirror` puts face i and its copy 2F-1-i into one chunk around the
    middle of the list (another wave of the same chunk), `repeat` puts them side by side (neighbouring lanes of one wave)."""
    F = len(f)
    return [("tile", np.tile(f, (3, 1)), np.arange(F)),
            ("mirror", np.concatenate([f, f[::-1]]), np.arange(F)),
            ("repeat", np.repeat(f, 2, axis=0), 2 * np.arange(F))]


def rotation(seed):
    """A rotation matrix drawn from the seed (QR of a Gaussian matrix, determinant +1)."""
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q
