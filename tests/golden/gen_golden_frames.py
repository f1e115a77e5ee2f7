"""Generate tests/golden/g33_frames.npz by running the reference's own frame-table code on the CPU (development container only,
like gen_golden_root_pose.py): get_near_far over pts_to_view, K2mat, K2inv, mat2K and near_far_to_bound of
nnutils/geom_utils.py, in fp32 and in float64 (torch's default dtype switched, since the reference's helpers allocate in the
default dtype), always with pts= (trimesh is not installed here), and banmo.save_latest_vars compiled on its own from the
syntax tree of nnutils/moda.py (the module cannot be imported here: absl flags, mcubes) and run against a stand-in object.
The near-far reset of forward_default (moda.py:485-491) is three lines inside a method that needs the whole model; its two
numpy lines are replayed literally here before the reference's get_near_far is called.

Inputs and outputs only.  Keys: `names` lists the cases; a case stores `<name>/pts`, `/rtk`, `/idk`, `/nf0`, `/tol`, optionally
`/rtk_all`, and the reference's `/nf32`, `/nf64` (and `/rtk32` after a patch).  The shape grid shares `grid/pts`, `grid/rtk`,
`grid/nf0` by prefix and stores `grid/<M>x<N>/nf32|nf64`.  `slv/<name>/...` are the save_latest_vars cases.

    python tests/golden/gen_golden_frames.py
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402

GRID_M = (1, 3, 64, 65, 257)
GRID_N = (1, 8, 32, 33, 63, 64, 65, 256, 257, 1025, 4096, 4097, 8193)    # 32 | 33: one lane a frame | a workgroup; 4096 | 4097: unsplit | split at small M


def save_latest_vars_of(geom):
    """banmo.save_latest_vars compiled from moda.py's syntax tree without importing the module."""
    tree = ast.parse(open(os.path.join(_ref_import.REF, "nnutils", "moda.py")).read())
    ns = {"torch": torch, "K2mat": geom.K2mat, "K2inv": geom.K2inv, "mat2K": geom.mat2K}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == "save_latest_vars":
            exec(compile(ast.Module([node], []), "moda.py", "exec"), ns)
    return ns["save_latest_vars"]


def poses(rng, M, tz=3.0):
    """(M,4,4) fp32: a random rotation, a translation with depth around tz, an intrinsics row."""
    q, _ = np.linalg.qr(rng.standard_normal((M, 3, 3)))
    rtk = np.zeros((M, 4, 4), np.float32)
    rtk[:, :3, :3] = q
    rtk[:, :3, 3] = rng.standard_normal((M, 3)) * 0.3 + np.asarray([0, 0, tz])
    rtk[:, 3] = np.abs(rng.standard_normal((M, 4))) * 50 + np.asarray([300, 500, 200, 250])
    return rtk


def run_ref(geom, nf0, rtk, idk, pts, tol, dt):
    torch.set_default_dtype(dt)
    try:
        nf = torch.from_numpy(np.asarray(nf0)).to(dt).clone()
        out = geom.get_near_far(nf, {"rtk": np.asarray(rtk), "idk": np.asarray(idk)}, tol_fac=tol, pts=np.asarray(pts))
        return out.numpy().copy()
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    _, _, geom, _ = _ref_import.import_reference()
    slv = save_latest_vars_of(geom)
    rng = np.random.default_rng(33)
    out, names = {}, []

    def case(name, pts, rtk, idk, nf0, tol=1.2, rtk_all=None):
        pts, rtk, idk, nf0 = (np.ascontiguousarray(a, np.float32) for a in (pts, rtk, idk, nf0))
        names.append(name)
        out.update({f"{name}/pts": pts, f"{name}/rtk": rtk, f"{name}/idk": idk, f"{name}/nf0": nf0, f"{name}/tol": np.asarray(tol)})
        tab = rtk
        if rtk_all is not None:                                          # moda.py:486-488, literally
            rtk_all = np.ascontiguousarray(rtk_all, np.float32)
            out[f"{name}/rtk_all"] = rtk_all
            latest_vars = {"rtk": rtk.copy(), "idk": idk}
            valid_rts = latest_vars["idk"].astype(bool)
            latest_vars["rtk"][valid_rts, :3] = rtk_all[valid_rts]
            tab = out[f"{name}/rtk32"] = latest_vars["rtk"]
        out[f"{name}/nf32"] = run_ref(geom, nf0, tab, idk, pts, tol, torch.float32)
        out[f"{name}/nf64"] = run_ref(geom, nf0, tab, idk, pts, tol, torch.float64)

    # the shape grid
    gp = (rng.standard_normal((max(GRID_N), 3)) * 0.4).astype(np.float32)
    gr = poses(rng, max(GRID_M))
    g0 = np.abs(rng.standard_normal((max(GRID_M), 2))).astype(np.float32)
    out.update({"grid/pts": gp, "grid/rtk": gr, "grid/nf0": g0, "grid/M": np.asarray(GRID_M), "grid/N": np.asarray(GRID_N)})
    for M in GRID_M:
        for N in GRID_N:
            ones = np.ones(M, np.float32)
            out[f"grid/{M}x{N}/nf32"] = run_ref(geom, g0[:M], gr[:M], ones, gp[:N], 1.2, torch.float32)
            out[f"grid/{M}x{N}/nf64"] = run_ref(geom, g0[:M], gr[:M], ones, gp[:N], 1.2, torch.float64)

    # where the extremes sit: first point, last point, last lane of the first wave, first lane of the second, for a frame of one
    # partial second wave (70) and one that wraps the workgroup's stride (330).  Identity rotation: the depth is p_z + T_z.
    M = 3
    eye = poses(rng, M)
    eye[:, :3, :3] = np.eye(3)
    nf0 = np.abs(rng.standard_normal((M, 2)))
    for N in (70, 330):
        for pos in sorted({0, 63, 64, N - 1}):
            for which, v in (("min", -2.0), ("max", 2.0)):
                p = rng.standard_normal((N, 3)) * 0.1
                p[pos, 2] = v
                case(f"place/{N}/{pos}/{which}", p, eye, np.ones(M), nf0)
    case("equal", np.tile(rng.standard_normal((1, 3)) * 0.2, (100, 1)), poses(rng, M), np.ones(M), nf0)
    case("behind", rng.standard_normal((100, 3)) * 0.2, poses(rng, M, tz=-10.0), np.ones(M), nf0)
    case("tol15", rng.standard_normal((40, 3)) * 0.2, poses(rng, M), np.ones(M), nf0, tol=1.5)

    # idk: mixed values with the pose patch, 2.0 rows (patched, not written), all unseen
    M = 9
    idk = np.asarray([1, 0, 2, 1, 0, 1, 2, 0, 1], np.float32)
    nf0 = np.abs(rng.standard_normal((M, 2)))
    for N in (8, 100):
        case(f"mixed/{N}", rng.standard_normal((N, 3)) * 0.3, poses(rng, M), idk, nf0, rtk_all=poses(rng, M, tz=4.0)[:, :3])
        case(f"unseen/{N}", rng.standard_normal((N, 3)) * 0.3, poses(rng, M), np.zeros(M), nf0, rtk_all=poses(rng, M, tz=4.0)[:, :3])
        case(f"mixed_nopatch/{N}", rng.standard_normal((N, 3)) * 0.3, poses(rng, M), idk, nf0)

    # NaN and inf
    M = 5
    nf0 = np.abs(rng.standard_normal((M, 2)))
    for N in (8, 100, 5000):
        p = rng.standard_normal((N, 3)) * 0.3
        p[N // 2, 1] = np.nan
        case(f"nan_point/{N}", p, poses(rng, M), np.ones(M), nf0)
        r = poses(rng, M)
        r[2, 2, 1] = np.nan
        case(f"nan_pose/{N}", rng.standard_normal((N, 3)) * 0.3, r, np.ones(M), nf0)
        r = poses(rng, M)
        r[1, 0, 3] = np.nan                                              # a NaN in row 0 reaches the depth through pinhole_cam's 0 * x
        case(f"nan_pose_x/{N}", rng.standard_normal((N, 3)) * 0.3, r, np.ones(M), nf0)
        p = rng.standard_normal((N, 3)) * 0.3
        p[N - 1, 2] = np.inf
        case(f"inf_point/{N}", p, poses(rng, M), np.ones(M), nf0)

    # the box of a mesh's bounds, its corners passed explicitly
    bounds = np.asarray([[-0.3, -0.2, -0.25], [0.3, 0.2, 0.25]], np.float32)
    corners = np.asarray([[bounds[i, 0], bounds[j, 1], bounds[k, 2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    out["box/bounds"] = bounds
    case("box", corners, poses(rng, 16), np.ones(16), np.zeros((16, 2)))
    out["bound32"] = geom.near_far_to_bound(torch.from_numpy(out["box/nf32"]))
    out["bound64"] = geom.near_far_to_bound(torch.from_numpy(out["box/nf64"]))

    # save_latest_vars: frames named once, twice and three times
    M = 10
    tabs = {"rtk": rng.standard_normal((M, 4, 4)).astype(np.float32), "rt_raw": rng.standard_normal((M, 3, 4)).astype(np.float32),
            "idk": np.asarray([0, 1, 0, 0, 1, 0, 0, 0, 0, 1], np.float32)}
    for name, fid in (("once", [3, 7, 0, 9]), ("twice", [3, 7, 3, 0]), ("thrice", [5, 2, 5, 8, 5, 2]), ("pairs", [4, 4, 6, 6, 4, 1, 6, 0])):
        fid = np.asarray(fid, np.int64)
        bs = len(fid)
        rtk = poses(rng, bs)
        kaug = (np.abs(rng.standard_normal((bs, 4))) + np.asarray([0.5, 0.8, 0.1, 0.2])).astype(np.float32)
        rt_raw = rng.standard_normal((bs, 3, 4)).astype(np.float32)
        out.update({f"slv/{name}/frameid": fid, f"slv/{name}/rtk": rtk, f"slv/{name}/kaug": kaug, f"slv/{name}/rt_raw": rt_raw})
        for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
            torch.set_default_dtype(dt)
            try:
                obj = types.SimpleNamespace(rtk=torch.from_numpy(rtk).to(dt), kaug=torch.from_numpy(kaug).to(dt), frameid=torch.from_numpy(fid),
                                            rt_raw=torch.from_numpy(rt_raw).to(dt),
                                            latest_vars={k: v.astype(np.float64 if tag == "64" else np.float32) for k, v in tabs.items()})
                slv(obj)
            finally:
                torch.set_default_dtype(torch.float32)
            for k in ("rtk", "rt_raw", "idk"):
                out[f"slv/{name}/out_{k}{tag}"] = obj.latest_vars[k]
    out.update({"slv/tab_rtk": tabs["rtk"], "slv/tab_rt_raw": tabs["rt_raw"], "slv/tab_idk": tabs["idk"],
                "slv/names": np.asarray(["once", "twice", "thrice", "pairs"])})
    out["names"] = np.asarray(names)

    path = os.path.join(HERE, "g33_frames.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
