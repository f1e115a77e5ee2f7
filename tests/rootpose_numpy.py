"""Float64 numpy restatement of the root-pose chain with hand-written gradients: the tails of RTHead / RTExplicit / RTExpMLP
(reference nnutils/nerf.py:307-344, 382-470), refine_rt / create_base_se3 / compute_rts / convert_root_pose
(nnutils/moda.py:1025-1033, 1419-1495), prepare_ray_cams (moda.py:1036-1046 over geom_utils.py:596-652), raycast's two lines
(geom_utils.py:763-766) and the NeRF-shaped MLP that feeds the tail (nerf.py:147-198, raw_feat, no direction input).

so3_exp restates pytorch3d's so3_exponential_map (absent from the reference tree, unpinned): theta = sqrt(clamp(sum(w * w),
min=1e-4)), R = sin(theta) / theta hat(w) + (1 - cos(theta)) / theta^2 hat(w)^2 + I; no gradient through a clamped theta.
`clamp` is the bound the clamp compares with: float32(1e-4) where the inputs are an fp32 run's (the default), 1e-4 for the
reference's own float64 run."""
import numpy as np

CLAMP32 = float(np.float32(1e-4))
BASE_Z = float(np.float32(0.3))          # create_base_se3 builds an fp32 tensor whatever follows


def hat(w):
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -w[..., 2], w[..., 1]
    K[..., 1, 0], K[..., 1, 2] = w[..., 2], -w[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -w[..., 1], w[..., 0]
    return K


def so3_exp(w, clamp=CLAMP32):
    w = np.asarray(w, np.float64)
    nrm = (w * w).sum(-1)
    th = np.sqrt(np.maximum(nrm, clamp))
    f1, f2 = np.sin(th) / th, (1 - np.cos(th)) / th ** 2
    K = hat(w)
    return f1[..., None, None] * K + f2[..., None, None] * (K @ K) + np.eye(3)


def so3_exp_bwd(w, G, clamp=CLAMP32):
    w = np.asarray(w, np.float64)
    nrm = (w * w).sum(-1)
    th = np.sqrt(np.maximum(nrm, clamp))
    s, c = np.sin(th), np.cos(th)
    f1, f2 = s / th, (1 - c) / th ** 2
    K = hat(w)
    K2 = K @ K
    D = f1[..., None, None] * G - f2[..., None, None] * (G @ K + K @ G)
    dw = np.stack([D[..., 2, 1] - D[..., 1, 2], D[..., 0, 2] - D[..., 2, 0], D[..., 1, 0] - D[..., 0, 1]], -1)
    df1 = (th * c - s) / th ** 2
    df2 = (th * s - 2 * (1 - c)) / th ** 3
    coef = ((G * K).sum((-1, -2)) * df1 + (G * K2).sum((-1, -2)) * df2) / th
    return dw + np.where(nrm >= clamp, coef, 0.0)[..., None] * w


def quat_to_matrix(q):
    r, i, j, k = (q[..., m] for m in range(4))
    ts = 2.0 / (q * q).sum(-1)
    o = np.stack([1 - ts * (j * j + k * k), ts * (i * j - k * r), ts * (i * k + j * r),
                  ts * (i * j + k * r), 1 - ts * (i * i + k * k), ts * (j * k - i * r),
                  ts * (i * k - j * r), ts * (j * k + i * r), 1 - ts * (i * i + j * j)], -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def quat_exp(q):
    q = np.asarray(q, np.float64)
    den = np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), 1e-12)
    return quat_to_matrix(q / den)


def quat_exp_bwd(q, G):
    q = np.asarray(q, np.float64)
    nrm = np.sqrt((q * q).sum(-1, keepdims=True))
    den = np.maximum(nrm, 1e-12)
    u = q / den
    r, i, j, k = (u[..., m] for m in range(4))
    g = G.reshape(G.shape[:-2] + (9,))
    g = [g[..., m] for m in range(9)]
    ts = 2.0 / (u * u).sum(-1)
    Gs = (-g[0] * (j * j + k * k) + g[1] * (i * j - k * r) + g[2] * (i * k + j * r) + g[3] * (i * j + k * r) - g[4] * (i * i + k * k)
          + g[5] * (j * k - i * r) + g[6] * (i * k - j * r) + g[7] * (j * k + i * r) - g[8] * (i * i + j * j))
    a = np.stack([-k * g[1] + j * g[2] + k * g[3] - i * g[5] - j * g[6] + i * g[7],
                  j * g[1] + k * g[2] + j * g[3] - 2 * i * g[4] - r * g[5] + k * g[6] + r * g[7] - 2 * i * g[8],
                  -2 * j * g[0] + i * g[1] + r * g[2] + i * g[3] + k * g[5] - r * g[6] + k * g[7] - 2 * j * g[8],
                  -2 * k * g[0] - r * g[1] + i * g[2] + r * g[3] - 2 * k * g[4] + j * g[5] + i * g[6] + j * g[7]], -1)
    du = ts[..., None] * a - (ts * ts * Gs)[..., None] * u
    free = (du - u * (du * u).sum(-1, keepdims=True)) / den
    return np.where(nrm >= 1e-12, free, du / den)


def head(rows, clamp=CLAMP32):
    """[t | rotation] rows, 7 columns (quaternion) or 6 (rotation vector) -> R (n,3,3), t (n,3)."""
    rows = np.asarray(rows, np.float64)
    R = quat_exp(rows[:, 3:7]) if rows.shape[1] == 7 else so3_exp(rows[:, 3:6], clamp)
    return R, rows[:, :3] * 0.1


def head_bwd(rows, gR, gt, clamp=CLAMP32):
    rows = np.asarray(rows, np.float64)
    dr = quat_exp_bwd(rows[:, 3:7], gR) if rows.shape[1] == 7 else so3_exp_bwd(rows[:, 3:6], gR, clamp)
    return np.concatenate([0.1 * gt, dr], -1)


def id_rows_sum(rows, ids, T, dtype=np.float64):
    """d_table (T, C) = sum of rows[i] over ids[i] == t in increasing i (in `dtype`: float32 gives the kernel's own sum)."""
    out = np.zeros((T, rows.shape[1]), dtype)
    for i, t in enumerate(np.asarray(ids).tolist()):
        if 0 <= t < T:
            out[t] = out[t] + rows[i].astype(dtype)
    return out


def create_base_se3(n):
    rt = np.zeros((n, 3, 4))
    rt[:, :3, :3] = np.eye(3)
    rt[:, 2, 3] = BASE_Z
    return rt


def refine_rt(rt_raw, R, t):
    out = np.array(rt_raw, np.float64)
    R0, t0 = out[:, :3, :3].copy(), out[:, :3, 3].copy()
    out[:, :3, 3] = t0 + (R0 @ t[..., None])[..., 0]
    out[:, :3, :3] = R0 @ R
    return out


def root_pose(se3=None, ids=None, delta=None, rt_raw=None, raw="base", obj_scale=1.0, ks=None, dataid=None, g=None,
              clamp=CLAMP32):
    """The fused tail.  raw: "none" (the module's own output), "base" (create_base_se3), "rows" (rt_raw (n,3|4,4)) or "by_id"
    (rt_raw (T,3|4,4)).  -> dict(rtk (n,4,4)) and, with g (n,4,4) given, d_rows, d_se3, d_delta, d_ks_rows, d_ks."""
    n = len(ids) if delta is None else len(delta)
    both = se3 is not None and delta is not None
    Rb, tb = np.broadcast_to(np.eye(3), (n, 3, 3)), np.zeros((n, 3))
    if se3 is not None:
        brows = np.asarray(se3, np.float64)[np.asarray(ids)]
        Rb, tb = head(brows, clamp)
        if both:
            Rb, tb = Rb * 10 - Rb * 9, tb * 10 - tb * 9
    if delta is not None:
        Rd, td = head(delta, clamp)
    if both:
        Rr, tr = Rb @ Rd, tb + (Rb @ td[..., None])[..., 0]
    elif delta is not None:
        Rr, tr = Rd, td
    else:
        Rr, tr = Rb, tb
    if raw == "none":
        R0, t0 = np.broadcast_to(np.eye(3), (n, 3, 3)), np.zeros((n, 3))
    elif raw == "base":
        R0, t0 = np.broadcast_to(np.eye(3), (n, 3, 3)), np.broadcast_to(np.array([0, 0, BASE_Z]), (n, 3))
    else:
        rr = np.asarray(rt_raw, np.float64)
        rr = rr[np.asarray(ids)] if raw == "by_id" else rr
        R0, t0 = rr[:, :3, :3], rr[:, :3, 3] / obj_scale
    rtk = np.zeros((n, 4, 4))
    rtk[:, :3, :3] = R0 @ Rr
    rtk[:, :3, 3] = t0 + (R0 @ tr[..., None])[..., 0]
    rtk[:, 3] = np.array([0, 0, 0, 1.0]) if ks is None else np.asarray(ks, np.float64)[np.asarray(dataid)]
    out = {"rtk": rtk}
    if g is None:
        return out
    g = np.asarray(g, np.float64)
    gR, gt = g[:, :3, :3], g[:, :3, 3]
    gRr, gtr = R0.transpose(0, 2, 1) @ gR, (R0.transpose(0, 2, 1) @ gt[..., None])[..., 0]
    if ks is not None:
        out["d_ks_rows"] = g[:, 3].copy()
        out["d_ks"] = id_rows_sum(g[:, 3], dataid, len(ks))
    if both:
        gRb = gRr @ Rd.transpose(0, 2, 1) + gtr[:, :, None] * td[:, None, :]
        gRd = Rb.transpose(0, 2, 1) @ gRr
        gtd = (Rb.transpose(0, 2, 1) @ gtr[..., None])[..., 0]
        out["d_rows"] = head_bwd(brows, 10 * gRb, 10 * gtr, clamp)
        out["d_delta"] = head_bwd(delta, gRd, gtd, clamp)
    elif se3 is not None:
        out["d_rows"] = head_bwd(brows, gRr, gtr, clamp)
    elif delta is not None:
        out["d_delta"] = head_bwd(delta, gRr, gtr, clamp)
    if se3 is not None:
        out["d_se3"] = id_rows_sum(out["d_rows"], ids, len(se3))
    return out


def rts12(rtk):
    """(n,4,4) -> the modules' (n,1,12) = [R (9) | t (3)]."""
    return np.concatenate([rtk[:, :3, :3].reshape(-1, 9), rtk[:, :3, 3]], -1)[:, None]


def rts12_bwd(g12):
    """gradient on (n,1,12) -> gradient on (n,4,4)."""
    g = np.zeros((g12.shape[0], 4, 4))
    g[:, :3, :3] = g12[:, 0, :9].reshape(-1, 3, 3)
    g[:, :3, 3] = g12[:, 0, 9:]
    return g


# ---- intrinsics and rays ---------------------------------------------------------------------------------------------------------
def K2mat(K):
    M = np.zeros((len(K), 3, 3))
    M[:, 0, 0], M[:, 1, 1], M[:, 0, 2], M[:, 1, 2], M[:, 2, 2] = K[:, 0], K[:, 1], K[:, 2], K[:, 3], 1
    return M


def K2inv(K):
    M = np.zeros((len(K), 3, 3))
    M[:, 0, 0], M[:, 1, 1], M[:, 0, 2], M[:, 1, 2], M[:, 2, 2] = 1 / K[:, 0], 1 / K[:, 1], -K[:, 2] / K[:, 0], -K[:, 3] / K[:, 1], 1
    return M


def mat2K(M):
    return np.stack([M[:, 0, 0], M[:, 1, 1], M[:, 0, 2], M[:, 1, 2]], -1)


def Kmatinv(M):
    return K2inv(mat2K(M))


def ray_cams(rtk, kaug, gR=None, gT=None, gK=None):
    rtk, kaug = np.asarray(rtk, np.float64), np.asarray(kaug, np.float64)
    P = K2inv(kaug) @ K2mat(rtk[:, 3])
    out = {"Rmat": rtk[:, :3, :3].copy(), "Tmat": rtk[:, :3, 3].copy(), "Kinv": Kmatinv(P)}
    if gR is None and gT is None and gK is None:
        return out
    d = np.zeros_like(rtk)
    if gR is not None:
        d[:, :3, :3] = gR
    if gT is not None:
        d[:, :3, 3] = gT
    if gK is not None:
        P00, P11, P02, P12 = P[:, 0, 0], P[:, 1, 1], P[:, 0, 2], P[:, 1, 2]
        dP00 = (gK[:, 0, 2] * P02 - gK[:, 0, 0]) / P00 ** 2
        dP11 = (gK[:, 1, 2] * P12 - gK[:, 1, 1]) / P11 ** 2
        d[:, 3, 0], d[:, 3, 1] = dP00 / kaug[:, 0], dP11 / kaug[:, 1]
        d[:, 3, 2], d[:, 3, 3] = -gK[:, 0, 2] / P00 / kaug[:, 0], -gK[:, 1, 2] / P11 / kaug[:, 1]
    out["d_rtk"] = d
    return out


def raycast(xys, Rmat, Tmat, Kinv, g_d=None, g_o=None):
    """geom_utils.py:763-766: rays_d = (Kinv [x, y, 1])^T R, rays_o = -T^T R; with g_d, g_o the gradients on R, T, Kinv."""
    xys = np.asarray(xys, np.float64)
    h = np.concatenate([xys, np.ones(xys.shape[:2] + (1,))], -1)          # (bs, ns, 3)
    c = h @ Kinv.transpose(0, 2, 1)                                       # (Kinv h)^T
    out = {"rays_d": c @ Rmat, "rays_o": np.broadcast_to(-(Tmat[:, None, :] @ Rmat), c.shape).copy()}
    if g_d is None:
        return out
    out["d_Rmat"] = c.transpose(0, 2, 1) @ g_d - Tmat[:, :, None] * g_o.sum(1)[:, None, :]
    out["d_Tmat"] = -(Rmat @ g_o.sum(1)[..., None])[..., 0]
    gc = g_d @ Rmat.transpose(0, 2, 1)
    out["d_Kinv"] = gc.transpose(0, 2, 1) @ h
    return out


# ---- the MLP in front of the tail ------------------------------------------------------------------------------------------------
def mlp(params, x, D=8, skips=(4,), g=None):
    """NeRF.forward with raw_feat and no direction input (nerf.py:147-198) on x (n, C) in float64.  -> out, and with g the
    gradients {name: array} of every weight and bias plus d_x."""
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    x = np.asarray(x, np.float64)
    acts, h = [], x
    for i in range(D):
        if i in skips:
            h = np.concatenate([x, h], -1)
        z = h @ p[f"xyz_encoding_{i+1}.0.weight"].T + p[f"xyz_encoding_{i+1}.0.bias"]
        acts.append((h, z))
        h = np.maximum(z, 0)
    fin = h @ p["xyz_encoding_final.weight"].T + p["xyz_encoding_final.bias"]
    zd = fin @ p["dir_encoding.0.weight"].T + p["dir_encoding.0.bias"]
    hd = np.maximum(zd, 0)
    out = hd @ p["rgb.0.weight"].T + p["rgb.0.bias"]
    if g is None:
        return out
    grads = {"rgb.0.weight": g.T @ hd, "rgb.0.bias": g.sum(0)}
    dz = (g @ p["rgb.0.weight"]) * (zd > 0)
    grads["dir_encoding.0.weight"], grads["dir_encoding.0.bias"] = dz.T @ fin, dz.sum(0)
    dfin = dz @ p["dir_encoding.0.weight"]
    grads["xyz_encoding_final.weight"], grads["xyz_encoding_final.bias"] = dfin.T @ h, dfin.sum(0)
    dh = dfin @ p["xyz_encoding_final.weight"]
    dx = np.zeros_like(x)
    for i in reversed(range(D)):
        hin, z = acts[i]
        dz = dh * (z > 0)
        grads[f"xyz_encoding_{i+1}.0.weight"], grads[f"xyz_encoding_{i+1}.0.bias"] = dz.T @ hin, dz.sum(0)
        dh = dz @ p[f"xyz_encoding_{i+1}.0.weight"]
        if i in skips:
            dx += dh[:, :x.shape[1]]
            dh = dh[:, x.shape[1]:]
    grads["d_x"] = dx + dh
    return out, grads


# ---- moda.py:1419-1495, restated (nnutils/moda.py cannot be imported without absl and mcubes) ------------------------------------
def compute_rts(se3, delta, num_fr, rt_raw=None, obj_scale=1.0, g=None):
    """-> (T,3,4) of the frames 0 .. num_fr - 1; delta (T, 6|7) the MLP's output for them (None: the exp basis)."""
    ids = np.arange(num_fr)
    g4 = None
    if g is not None:
        g4 = np.zeros((num_fr, 4, 4))
        g4[:, :3] = g
    out = root_pose(se3, ids, delta, rt_raw, "base" if rt_raw is None else "rows", obj_scale, g=g4)
    out["rt"] = out["rtk"][:, :3]
    return out


def convert_root_pose(se3, delta, frameid, dataid, ks, rtk=None, obj_scale=1.0, g=None):
    return root_pose(se3, frameid, delta, rtk, "base" if rtk is None else "rows", obj_scale, ks, dataid, g)
