"""Float64 restatement of the frame tables of moda_amd/frame_state.py: banmo.save_latest_vars (reference nnutils/moda.py:1497-1513),
the pose patch of forward_default (:485-488), get_near_far over pts_to_view (nnutils/geom_utils.py:1105-1155) and
near_far_to_bound (:1185-1193).  Beside each value the functions return a running bound on what an fp32 evaluation of the
same operations may differ by, as tests/composite_numpy.py does; u = 2^-24 is fp32's unit round-off.

The planes.  For a frame with third pose row (R2, T2) and S = max_n(|R2| . |p_n| + |T2|):
  z_n = ((p0 R20 + p1 R21) + p2 R22) + T2: three rounded products, whose errors u |term| add up to at most u S, and three rounded
        sums, each of a partial sum no larger than S, so at most u S each: |z_n - fl(z_n)| <= 4 u S to first order.
        pinhole_cam's  x 0 + y 0 + z 1  is exact for finite x and y.
  pmin, pmax inherit 4 u S each (min and max select, they do not round).
  d = pmax - pmin: 8 u S inherited + u |d| <= 2 u S of its own rounding -> 10 u S.
  delta = d * f, f = fp32(tol_fac - 1): f (10 u S) inherited + u f |d| for f's own rounding + u f |d| for the product
        -> f (10 + 2 + 2) u S = 14 f u S.
  near = pmin - delta: 4 u S + 14 f u S + u |near| <= u S (1 + 2 f) of its own rounding -> (5 + 16 f) u S.
  (5 + 16 f) <= c (1 + 2 f) for every f >= 0 with c = 8, hence   bound = 8 u S (1 + 2 (tol_fac - 1)),
  plus u 1e-3 for the clamp's constant, which fp32 rounds.  An FMA-contracted or differently ordered dot product (torch's
  matmul) rounds no more often than this, so the reference's fp32 run obeys the same bound.

The composed intrinsics.  a = 1 / k0 (one rounding), a fx (one more), c = -k2 / k0 (one), a px + c (one more): three rounded
operations on any path to an entry, each relative to a magnitude <= |a| |px| + |c|, so bound = 3 u (|a| |v| + |c|) with v the
focal length (c term absent) or the principal point.
"""
import itertools

import numpy as np

U = 2.0 ** -24
C_PLANE = 8.0            # derived above


def compose_k(k, kaug):
    """mat2K(K2inv(kaug) @ K2mat(k)) for rows k, kaug (bs,4) -> (row (bs,4), bound (bs,4))."""
    k, kaug = np.asarray(k, np.float64), np.asarray(kaug, np.float64)
    a, b = 1.0 / kaug[:, 0], 1.0 / kaug[:, 1]
    c, d = -kaug[:, 2] / kaug[:, 0], -kaug[:, 3] / kaug[:, 1]
    row = np.stack([a * k[:, 0], b * k[:, 1], a * k[:, 2] + c, b * k[:, 3] + d], 1)
    bound = 3 * U * np.stack([np.abs(a * k[:, 0]), np.abs(b * k[:, 1]), np.abs(a * k[:, 2]) + np.abs(c),
                              np.abs(b * k[:, 3]) + np.abs(d)], 1)
    return row, bound


def last_occurrence(frameid, M):
    """-> (ids, src): the frames in [0, M) a batch names and, for each, the LAST batch index naming it (numpy's fancy assignment
    keeps the last occurrence); ids outside [0, M) are dropped (-> their count as third value)."""
    frameid = np.asarray(frameid, np.int64)
    last = {}
    refused = 0
    for b, f in enumerate(frameid.tolist()):
        if 0 <= f < M:
            last[f] = b
        else:
            refused += 1
    ids = np.asarray(sorted(last), np.int64)
    return ids, np.asarray([last[f] for f in ids.tolist()], np.int64), refused


def save_latest_vars(tables, rtk, kaug, rt_raw, frameid):
    """tables: dict rtk (M,4,4), rt_raw (M,3,4), idk (M,) -> (new tables (float64 copies), bound on rtk's row 3 (M,4), refused)."""
    out = {k: np.array(tables[k], np.float64) for k in ('rtk', 'rt_raw', 'idk')}
    M = out['rtk'].shape[0]
    rtk = np.array(rtk, np.float64)
    row, bnd = compose_k(rtk[:, 3], kaug)
    rtk[:, 3] = row
    ids, src, refused = last_occurrence(frameid, M)
    bound = np.zeros((M, 4))
    out['rtk'][ids] = rtk[src]
    out['rt_raw'][ids] = np.asarray(rt_raw, np.float64)[src]
    out['idk'][ids] = 1
    bound[ids] = bnd[src]
    return out, bound, refused


def patch_poses(rtk, idk, rtk_all):
    """moda.py:486-488: rows [:3] of the frames with idk.astype(bool) become rtk_all's -> a float64 copy."""
    out = np.array(rtk, np.float64)
    valid = np.asarray(idk).astype(bool)
    out[valid, :3] = np.asarray(rtk_all, np.float64)[valid]
    return out


def depths(pts, rtk):
    """pts_to_view's last coordinate (M,N): obj_to_cam, then pinhole_cam's product with K2mat^T = x 0 + y 0 + z 1 (NaN where x or
    y is not finite, as the reference's matmul gives)."""
    pts, rtk = np.asarray(pts, np.float64), np.asarray(rtk, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        cam = np.einsum('nj,mij->mni', pts, rtk[:, :3, :3]) + rtk[:, None, :3, 3]
        # the einsum sums NaN-free rows exactly as a loop does; a 0 * inf inside it is the reference's NaN too
        return cam[..., 0] * 0.0 + cam[..., 1] * 0.0 + cam[..., 2]


def get_near_far(near_far, rtk, idk, pts, tol_fac=1.2):
    """-> (near_far (M,2) float64 copy updated where idk == 1, bound (M,2): 0 on rows that keep their bits)."""
    out = np.array(near_far, np.float64)
    rtk, idk, pts = np.asarray(rtk, np.float64), np.asarray(idk, np.float64), np.asarray(pts, np.float64)
    z = depths(pts, rtk)
    nan = np.isnan(z).any(1)
    with np.errstate(invalid='ignore', over='ignore'):
        pmax = np.where(nan, np.nan, np.fmax.reduce(z, 1))          # torch's max / min propagate NaN
        pmin = np.where(nan, np.nan, np.fmin.reduce(z, 1))
        f = tol_fac - 1
        delta = (pmax - pmin) * f
        near, far = pmin - delta, pmax + delta
        clamp = lambda v: np.where(np.isnan(v), v, np.maximum(v, 1e-3))
        near, far = clamp(near), clamp(far)
        fin = np.where(np.isfinite(pts), pts, 0.0)
        S = (np.abs(fin)[None] * np.abs(np.nan_to_num(rtk[:, None, 2, :3], posinf=0.0, neginf=0.0))).sum(-1).max(1) + np.abs(
            np.nan_to_num(rtk[:, 2, 3], posinf=0.0, neginf=0.0))
    b = C_PLANE * U * S * (1 + 2 * abs(f)) + U * 1e-3
    sel = idk == 1
    out[sel, 0], out[sel, 1] = near[sel], far[sel]
    bound = np.zeros_like(out)
    bound[sel] = b[sel, None]
    return out, bound


def reset_near_far(near_far, rtk, idk, rtk_all, pts, tol_fac=1.2):
    """moda.py:485-491 -> (rtk patched, near_far, bound)."""
    rtk = patch_poses(rtk, idk, rtk_all)
    nf, bound = get_near_far(near_far, rtk, idk, pts, tol_fac)
    return rtk, nf, bound


def box_corners(bounds):
    b = np.asarray(bounds, np.float64).reshape(2, 3)
    return np.asarray([[b[i, 0], b[j, 1], b[k, 2]] for i, j, k in itertools.product((0, 1), repeat=3)])


def near_far_to_bound(near_far):
    nf = np.asarray(near_far, np.float64)
    return (nf[:, 1] - nf[:, 0]).mean() / 2
