"""float64 numpy restatements of moda_amd/cams.py (test infrastructure, like the other *_numpy.py): save_cams' fill rule,
align_sim3 with scipy's Rotation.from_matrix / mean restated from its published algorithm, visual_hull_align, the rank-count
median, the camera glyphs, and rtk_invert / rtk_compose / rot_angle.  The hull's scores follow the kernel's order of operations
(every product and sum on its own, the views in index order), so float64 against float64 they agree to the last bits."""
import numpy as np

F32 = np.float32


# ---- rigid transforms ---------------------------------------------------------------------------------------------------------
def rtk_invert(rtk, B):
    r = np.asarray(rtk, np.float64).reshape(-1, B, 12)
    Ri = r[..., :9].reshape(-1, B, 3, 3).transpose(0, 1, 3, 2)
    ti = -np.matmul(Ri, r[..., 9:12, None])[..., 0]
    return np.concatenate([Ri.reshape(-1, B, 9), ti], -1).reshape(np.shape(rtk))


def rtk_to_4x4(rtk):
    r = np.asarray(rtk, np.float64).reshape(-1, 12)
    out = np.tile(np.eye(4), (len(r), 1, 1))
    out[:, :3, :3], out[:, :3, 3] = r[:, :9].reshape(-1, 3, 3), r[:, 9:]
    return out


def rtk_compose(a, b):
    m = np.matmul(rtk_to_4x4(a), rtk_to_4x4(b))
    return np.concatenate([m[:, :3, :3].reshape(-1, 9), m[:, :3, 3]], -1).reshape(np.shape(a))


def rot_angle(mat, eps=1e-4):
    mat = np.asarray(mat, np.float64)
    cos = (mat[..., 0, 0] + mat[..., 1, 1] + mat[..., 2, 2] - 1) / 2
    return np.arccos(np.clip(cos, -1 + eps, 1 - eps))


# ---- save_cams ----------------------------------------------------------------------------------------------------------------
def fill_reference_loop(rtk, is_valid, frame_offset):
    """A literal transcription of train_utils.py:747-761 (np.where and argmin included): the sequence name of frame i is the
    index of its video.  -> (rtk_filled, src)."""
    rtk = np.array(rtk, copy=True)
    valid_ids = np.asarray(is_valid, bool)
    length = len(rtk)
    seq_of = np.zeros(length, np.int64)
    for v in range(len(frame_offset) - 1):
        seq_of[frame_offset[v]:frame_offset[v + 1]] = v
    src = np.arange(length)
    for i in range(length):
        seq_idx = np.asarray([seq_of[i] == seq_of[j] for j in range(length)]) if length < 400 else seq_of == seq_of[i]
        valid_ids_seq = np.where(valid_ids * seq_idx)[0]
        if len(valid_ids_seq) > 0 and not valid_ids[i]:
            closest_valid_idx = valid_ids_seq[np.abs(i - valid_ids_seq).argmin()]
            rtk[i][:3, :3] = rtk[closest_valid_idx][:3, :3]
            src[i] = closest_valid_idx
    return rtk, src


def fill_invalid_rotations(rtk, is_valid, frame_offset):
    """The last-valid-to-the-left / first-valid-to-the-right rule -> (rtk_filled, src)."""
    rtk = np.array(rtk, copy=True)
    valid = np.asarray(is_valid, bool)
    src = np.arange(len(rtk))
    for v in range(len(frame_offset) - 1):
        lo, hi = frame_offset[v], frame_offset[v + 1]
        left, last = np.full(hi - lo, -1), -1
        for i in range(lo, hi):
            last = i if valid[i] else last
            left[i - lo] = last
        nxt = -1
        for i in range(hi - 1, lo - 1, -1):
            nxt = i if valid[i] else nxt
            l, r = left[i - lo], nxt
            if valid[i] or (l < 0 and r < 0):
                continue
            src[i] = l if r < 0 or (l >= 0 and i - l <= r - i) else r
    rtk[:, :3, :3] = rtk[src, :3, :3]
    return rtk, src


def save_cams(rtk, is_valid, data_offset, obj_scale, tab_rtk, tab_rt_raw, unc_filter=True):
    """train_utils.py:744-791 on arrays (fp32 in, fp32 arithmetic: one product a translation entry) -> (rtk_out, src, n_valid,
    rows, tab_rtk, tab_rt_raw); the tables are copies."""
    rtk = np.asarray(rtk, F32)
    nv = len(data_offset) - 1
    off = [data_offset[v] - v for v in range(nv + 1)]
    out, src = fill_invalid_rotations(rtk, is_valid, off) if unc_filter else (rtk.copy(), np.arange(len(rtk)))
    out[:, :3, 3] = out[:, :3, 3] * F32(obj_scale)
    tab_rtk, tab_rt_raw = np.array(tab_rtk, copy=True), np.array(tab_rt_raw, copy=True)
    rows = np.zeros(len(rtk), np.int64)
    n_valid = np.zeros(nv, np.int64)
    for v in range(nv):
        n_valid[v] = np.asarray(is_valid, bool)[off[v]:off[v + 1]].sum()
        for i in range(off[v], off[v + 1]):
            rows[i] = i + v
            for row in (i + v, i + v + 1) if i == off[v + 1] - 1 else (i + v,):
                tab_rt_raw[row] = out[i, :3, :4]
                tab_rtk[row, :3, :3] = out[i, :3, :3]
    return out, src, n_valid, rows, tab_rtk, tab_rt_raw


# ---- align_sim3 ---------------------------------------------------------------------------------------------------------------
def mat_to_quat(M):
    """scipy's Rotation.from_matrix for one matrix -> (x, y, z, w), normalised."""
    tr = M[0, 0] + M[1, 1] + M[2, 2]
    dec = [M[0, 0], M[1, 1], M[2, 2], tr]
    ch = int(np.argmax(dec))
    q = np.zeros(4)
    if ch == 3:
        q[:] = [M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1], 1 + tr]
    else:
        i = ch
        j = (i + 1) % 3
        k = (j + 1) % 3
        q[i] = 1 - tr + 2 * M[i, i]
        q[j] = M[j, i] + M[i, j]
        q[k] = M[k, i] + M[i, k]
        q[3] = M[k, j] - M[j, k]
    return q / np.sqrt((q * q).sum())


def quat_to_mat(q):
    x, y, z, w = q
    return np.asarray([[x * x - y * y - z * z + w * w, 2 * (x * y - z * w), 2 * (x * z + y * w)],
                       [2 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), -x * x - y * y + z * z + w * w]])


def mean_rotation(mats):
    """scipy's Rotation.mean -> (matrix, eigenvalues ascending): the eigenvector of the largest eigenvalue of sum q q^T."""
    K = np.zeros((4, 4))
    for M in mats:
        q = mat_to_quat(M)
        K += np.outer(q, q)
    lam, vec = np.linalg.eigh(K)
    return quat_to_mat(vec[:, -1]), lam


def median_rank(x):
    """np.median by the rank-count rule: rank(i) = #{j: x[j] < x[i], or x[j] == x[i] and j < i}; the float64 mean of the elements
    of rank (m - 1) // 2 and m // 2."""
    x = np.asarray(x)
    m = len(x)
    if m == 0:
        return np.nan
    idx = np.arange(m)
    rank = ((x[None, :] < x[:, None]) | ((x[None, :] == x[:, None]) & (idx[None, :] < idx[:, None]))).sum(1)
    return 0.5 * (float(x[rank == (m - 1) // 2][0]) + float(x[rank == m // 2][0]))


def align_sim3(a, b, is_inlier=None, err_valid=None):
    """geom_utils.py:1463-1514 on copies, float64 -> dict(b, rotation, scale, so3_err (fp32 degrees), stats (max, median, mean,
    unbiased std), used, fallback, zero_norm, eig)."""
    a, b = np.asarray(a, np.float64), np.array(b, np.float64, copy=True)
    n = len(a)
    dso3 = np.matmul(b[:, :3, :3].transpose(0, 2, 1), a[:, :3, :3])
    nb = np.sqrt((b[:, :3, 3] ** 2).sum(-1))
    with np.errstate(all="ignore"):
        dscale = np.sqrt((a[:, :3, 3] ** 2).sum(-1)) / nb
    used = np.ones(n, bool)
    fallback = False
    if is_inlier is not None:
        used = np.array(is_inlier, bool, copy=True)
        if used.sum() == 0:
            used[np.argmin(err_valid)] = True
            fallback = True
    R, lam = mean_rotation(dso3[used])
    scale = dscale[used].mean()
    b[:, :3, :3] = np.matmul(b[:, :3, :3], R[None])
    b[:, :3, 3] = b[:, :3, 3] * scale
    err = (rot_angle(np.matmul(a[:, :3, :3], b[:, :3, :3].transpose(0, 2, 1))) / np.pi * 180).astype(F32)
    e64 = err.astype(np.float64)
    with np.errstate(all="ignore"):
        std = np.sqrt(((e64 - e64.mean()) ** 2).sum() / (n - 1)) if n > 1 else np.nan
    return dict(b=b, rotation=R, scale=scale, so3_err=err, stats=np.asarray([err.max(), median_rank(err), e64.mean(), std]),
                used=used, fallback=fallback, zero_norm=int((nb == 0).sum()), eig=lam[::-1][:2])


# ---- visual hull --------------------------------------------------------------------------------------------------------------
def hull_rows(rtk, kaug):
    """Per view, in fp32 and the reference's order: kmat = mat2K(K2inv(kaug) K2mat(rtk[:,3])) (V,4), the camera centres
    c = -R^T t (V,3), and bound = the mean of |c| over all 3 V entries (a float64 sum rounded once)."""
    r, ka = np.asarray(rtk, F32), np.asarray(kaug, F32)
    ix, iy = F32(1) / ka[:, 0], F32(1) / ka[:, 1]
    ox, oy = -ka[:, 2] / ka[:, 0], -ka[:, 3] / ka[:, 1]
    kmat = np.stack([ix * r[:, 3, 0], iy * r[:, 3, 1], ix * r[:, 3, 2] + ox, iy * r[:, 3, 3] + oy], -1).astype(F32)
    R, t = r[:, :3, :3], r[:, :3, 3]
    c = np.stack([-((R[:, 0, a] * t[:, 0] + R[:, 1, a] * t[:, 1]) + R[:, 2, a] * t[:, 2]) for a in range(3)], -1).astype(F32)
    bound = F32(np.abs(c).astype(np.float64).sum() / (3 * len(r)))
    return kmat, c, bound


def lattice(bound, G):
    """float32(np.linspace(-bound, bound, G)) evaluated in float64 from the fp32 bound."""
    return np.linspace(float(-F32(bound)), float(F32(bound)), G).astype(F32)


def hull_scores(rtk, kaug, masks, G):
    """-> (scores (G^3,) float64, points (G^3,3) fp32 values as float64, non-finite samples, kmat, c, bound)."""
    V, h, w = masks.shape
    r = np.asarray(rtk, F32)[:V].astype(np.float64)
    kmat, c, bound = hull_rows(np.asarray(rtk, F32)[:V], kaug)
    k = kmat.astype(np.float64)
    pts = lattice(bound, G).astype(np.float64)
    X, Y, Z = (g.reshape(-1) for g in np.meshgrid(pts, pts, pts, indexing="ij"))
    m = np.asarray(masks).astype(np.float64)
    score = np.zeros(G ** 3)
    bad = 0
    for v in range(V):
        R, t = r[v, :3, :3], r[v, :3, 3]
        with np.errstate(all="ignore"):
            xc = ((R[0, 0] * X + R[0, 1] * Y) + R[0, 2] * Z) + t[0]
            yc = ((R[1, 0] * X + R[1, 1] * Y) + R[1, 2] * Z) + t[1]
            zc = ((R[2, 0] * X + R[2, 1] * Y) + R[2, 2] * Z) + t[2]
            den = 1e-6 + zc
            px, py = (k[v, 0] * xc + k[v, 2] * zc) / den, (k[v, 1] * yc + k[v, 3] * zc) / den
            gx, gy = px / w * 2.0 - 1.0, py / h * 2.0 - 1.0
            fx, fy = ((gx + 1.0) * w - 1.0) / 2.0, ((gy + 1.0) * h - 1.0) / 2.0
        fin = np.isfinite(fx) & np.isfinite(fy)
        bad += int((~fin).sum())
        fx, fy = np.where(fin, fx, -10.0), np.where(fin, fy, -10.0)
        x0, y0 = np.floor(fx), np.floor(fy)
        ok = (x0 >= -1) & (x0 <= w - 1) & (y0 >= -1) & (y0 <= h - 1)
        xi, yi = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)
        ax, ay, bx, by = fx - x0, fy - y0, (x0 + 1.0) - fx, (y0 + 1.0) - fy
        s = np.zeros(G ** 3)
        for dy, dx, wt in ((0, 0, bx * by), (0, 1, ax * by), (1, 0, bx * ay), (1, 1, ax * ay)):
            xx, yy = xi + dx, yi + dy
            inside = ok & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            val = m[v, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
            s = np.where(inside, s + val * wt, s)
        score = score + s
    return score, np.stack([X, Y, Z], -1), bad, kmat, c, bound


def visual_hull_align(rtk, kaug, masks, G=64):
    """geom_utils.py:1552-1608 -> dict(rtk (V,4,4) float64, scores, selected (G^3,) bool, bound, empty, nonfinite)."""
    V = masks.shape[0]
    score, pts, bad, _, c, bound = hull_scores(rtk, kaug, masks, G)
    sel = score > 0.8 * V
    out = np.asarray(rtk, F32)[:V].astype(np.float64)
    if sel.any():
        centre = pts[sel].sum(0) / sel.sum()
        d = c.astype(np.float64) - centre[None]
        R = out[:, :3, :3]
        out[:, :3, 3] = -((R[:, :, 0] * d[:, 0:1] + R[:, :, 1] * d[:, 1:2]) + R[:, :, 2] * d[:, 2:3])
    return dict(rtk=out, scores=score, selected=sel, bound=bound, empty=not sel.any(), nonfinite=bad)


# ---- glyphs -------------------------------------------------------------------------------------------------------------------
BOX_FACES = np.asarray([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                        [1, 5, 7], [1, 7, 3]], np.int64)


def box(lo, hi):
    return np.asarray([[(hi if a else lo)[0], (hi if b else lo)[1], (hi if c else lo)[2]] for a in (0, 1) for b in (0, 1) for c in (0, 1)],
                      np.float64)


def draw_cams(all_cam, color='cool', color_list=None):
    """-> (vertices (n 32, 3) float64, faces (n 48, 3), colors (n 32, 4) uint8, scale = the median of the non-zero |t|)."""
    cams = np.asarray(all_cam, F32)
    n = len(cams)
    t64 = cams[:, :3, 3].astype(np.float64)
    norms = np.sqrt((t64[:, 0] * t64[:, 0] + t64[:, 1] * t64[:, 1]) + t64[:, 2] * t64[:, 2]).astype(F32)
    scale = F32(median_rank(norms[norms > 0]))
    radius = float(F32(0.02) * scale)
    parts = [box([-.5] * 3, [.5] * 3)]
    for a in range(3):
        lo, hi = [-0.1] * 3, [0.1] * 3
        lo[a], hi[a] = 0.0, 5.0
        parts.append(box(lo, hi))
    tmpl = np.concatenate(parts).astype(F32).astype(np.float64)
    x = np.arange(n) / float(n) if color_list is None else np.asarray(color_list, np.float64)
    rgb = {'cool': np.stack([x, 1 - x, np.ones(n)], -1), 'gray': np.stack([x, x, x], -1)}[color]
    own = np.concatenate([np.floor(255 * rgb + 0.5), np.full((n, 1), 255.)], -1).astype(np.uint8)
    axis = np.asarray([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255]], np.uint8)
    verts = np.zeros((n, 32, 3))
    colors = np.zeros((n, 32, 4), np.uint8)
    R = cams[:, :3, :3].astype(np.float64)
    for j in range(n):
        g = radius * tmpl - t64[j][None]
        verts[j] = np.matmul(g, R[j])                                                  # rows: R^T (radius v - t)
        colors[j, :8] = own[j]
        colors[j, 8:] = np.repeat(axis, 8, 0)
    faces = np.concatenate([np.concatenate([BOX_FACES + 8 * i for i in range(4)]) + 32 * j for j in range(n)])
    return verts.reshape(-1, 3), faces, colors.reshape(-1, 4), float(scale)
