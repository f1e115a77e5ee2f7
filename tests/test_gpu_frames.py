"""The frame tables on the GPU (moda_amd/frame_state.py, csrc/frames_kernels.hip) against the float64 oracle tests/frames_numpy.py
within the bound it states, and against the reference's own fp32 records (tests/golden/g33_frames.npz) within twice that bound
(the reference's fp32 run and the kernel may each sit a whole bound from the float64 value, on opposite sides).  Rows that are
not to be written, copies and the order-free min / max are compared bit for bit."""
import os
import types

import numpy as np
import pytest
import torch

import frames_numpy as fn
import moda_amd
from moda_amd import frame_state as FS
from test_frames_oracle import CASES, G, GRID, case_inputs, close

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(pts, rtk, idk, nf0, tol=1.2, rtk_all=None, splits=0):
    st = FS.FrameState(len(rtk), DEV)
    st.rtk.copy_(T(rtk))
    st.idk.copy_(T(idk))
    nf = T(nf0).clone()
    out = FS.get_near_far(nf, st, tol, T(pts), rtk_all=None if rtk_all is None else T(rtk_all), splits=splits)
    assert out is nf
    return nf.cpu().numpy(), st


@pytest.mark.parametrize("M,N", GRID)
def test_near_far_on_the_shape_grid(M, N):
    pts, rtk, nf0 = G["grid/pts"][:N], G["grid/rtk"][:M], G["grid/nf0"][:M]
    want, bound = fn.get_near_far(nf0, rtk, np.ones(M), pts)
    got, st = run(pts, rtk, np.ones(M), nf0)
    print(f"M={M} N={N} splits={FS.near_far_splits(N, M)} excess over the bound {close(got, want, bound):.3e}")
    assert close(got, want, bound) <= 0
    assert close(got, G[f"grid/{M}x{N}/nf32"], 2 * bound) <= 0
    assert st.status.cpu().tolist() == [0, 0, 0, 0]
    assert np.array_equal(bits(st.rtk), bits(rtk))                       # without rtk_all the pose table is only read


@pytest.mark.parametrize("name", CASES)
def test_near_far_cases(name):
    """Placement of the extremes, equal points, points behind the camera, mixed / 2.0 / zero idk with the pose patch, NaN and
    +inf inputs."""
    pts, rtk_p, idk, nf0, tol = case_inputs(name)
    rtk_all = G[name + "/rtk_all"] if name + "/rtk_all" in G.files else None
    want, bound = fn.get_near_far(nf0, rtk_p, idk, pts, tol)
    got, st = run(pts, G[name + "/rtk"], idk, nf0, tol, rtk_all)
    assert close(got, want, bound) <= 0
    assert close(got, G[name + "/nf32"], 2 * bound) <= 0
    keep = idk != 1
    assert np.array_equal(bits(got[keep]), bits(nf0[keep]))              # idk 0 and idk 2.0 rows keep their bits
    if rtk_all is not None:
        assert np.array_equal(bits(st.rtk), bits(G[name + "/rtk32"]))    # rows [:3] patched where idk != 0, row 3 kept
        assert np.array_equal(bits(st.rtk[:, 3]), bits(G[name + "/rtk"][:, 3]))
    n_nan = int(np.isnan(want).any(1).sum())
    assert int(st.status[0]) == n_nan and int(st.status[1]) == 0
    if name.startswith("nan_pose"):
        assert n_nan == 1
    if name.startswith(("nan_point", "inf_point")):                      # the reference's 0 * inf: every seen frame is NaN
        assert n_nan == len(idk)
    if name.startswith("behind"):
        assert np.array_equal(bits(got), bits(np.full_like(got, 1e-3)))
    if name == "equal":
        assert np.array_equal(got[:, 0], got[:, 1])
    if n_nan:
        with pytest.raises(RuntimeError, match="NaN near / far"):
            st.check()
    st.check()                                                           # (zeroed by the check before)


@pytest.mark.parametrize("M,N,forced", [(3, 8193, (1, 2, 7, 256)), (1, 4097, (1, 2, 3)), (65, 5000, (1, 2, 5)), (5, 33, (1, 2, 33))])
def test_split_and_unsplit_give_the_same_bits(M, N, forced):
    pts, rtk, nf0 = G["grid/pts"][:N], G["grid/rtk"][:M], G["grid/nf0"][:M]
    idk = np.ones(M)
    base, _ = run(pts, rtk, idk, nf0)                                    # the library's own choice
    again, _ = run(pts, rtk, idk, nf0)
    assert np.array_equal(bits(base), bits(again))
    for s in forced:
        a, _ = run(pts, rtk, idk, nf0, splits=s)
        b, _ = run(pts, rtk, idk, nf0, splits=s)
        assert np.array_equal(bits(a), bits(base)) and np.array_equal(bits(b), bits(base)), s
    p = np.array(G["nan_point/5000/pts"])                                # a NaN in one range reaches the frame through the partials
    a, st = run(p, G["nan_point/5000/rtk"], np.ones(5), G["nan_point/5000/nf0"], splits=5)
    assert np.isnan(a).all() and int(st.status[0]) == 5
    with pytest.raises(ValueError, match="splits"):
        run(pts[:8], rtk, idk, nf0, splits=2)


def _model(name, state):
    p = "slv/" + name
    return types.SimpleNamespace(rtk=T(G[p + "/rtk"]), kaug=T(G[p + "/kaug"]), rt_raw=T(G[p + "/rt_raw"]),
                                 frameid=T(G[p + "/frameid"], torch.int64), latest_vars=state)


def _slv_state():
    return FS.FrameState.from_vars({k: G["slv/tab_" + k] for k in ("rtk", "rt_raw", "idk")}, None, DEV)


@pytest.mark.parametrize("name", [str(n) for n in G["slv/names"]])
def test_save_latest_vars(name):
    p = "slv/" + name
    tabs = {k: G["slv/tab_" + k] for k in ("rtk", "rt_raw", "idk")}
    want, bound, _ = fn.save_latest_vars(tabs, G[p + "/rtk"], G[p + "/kaug"], G[p + "/rt_raw"], G[p + "/frameid"])
    runs = []
    for _ in range(2):
        st = _slv_state()
        assert FS.save_latest_vars(_model(name, st)) is st
        runs.append([bits(st.rtk), bits(st.rt_raw), bits(st.idk)])
        st.check()
    assert all(np.array_equal(a, b) for a, b in zip(*runs))              # duplicates: the same row on every run
    rtk = st.rtk.cpu().numpy()
    ref = G[p + "/out_rtk32"]
    assert np.array_equal(bits(rtk[:, :3]), bits(ref[:, :3]))            # rows 0-2 (last occurrence) and untouched frames: exact
    assert np.array_equal(bits(st.rt_raw), bits(G[p + "/out_rt_raw32"]))
    assert np.array_equal(st.idk.cpu().numpy(), G[p + "/out_idk32"])     # set only on named frames, others as before
    assert (np.abs(rtk[:, 3].astype(np.float64) - want["rtk"][:, 3]) <= bound).all()
    assert (np.abs(rtk[:, 3].astype(np.float64) - ref[:, 3]) <= 2 * bound).all()
    named = np.unique(G[p + "/frameid"])
    rest = np.setdiff1d(np.arange(len(rtk)), named)
    assert np.array_equal(bits(rtk[rest]), bits(tabs["rtk"][rest]))


def test_save_latest_vars_refuses_ids_outside_the_tables():
    st = _slv_state()
    m = _model("twice", st)
    M = st.num_frames
    before = [bits(st.rtk), bits(st.rt_raw), bits(st.idk)]
    m.frameid = T(np.asarray([-1, M, M + 5, -7]), torch.int64)
    FS.save_latest_vars(m)
    assert st.status.cpu().tolist() == [0, 4, 0, 0]
    assert all(np.array_equal(a, b) for a, b in zip(before, [bits(st.rtk), bits(st.rt_raw), bits(st.idk)]))
    with pytest.raises(RuntimeError, match=r"4 frame id\(s\) outside \[0, 10\)"):
        st.check()
    m.frameid = T(np.asarray([-1, 2, M, 2]), torch.int64)                # the valid entries are still written, last occurrence
    FS.save_latest_vars(m)
    assert int(st.status[1]) == 2 and float(st.idk[2]) == 1.0
    assert np.array_equal(bits(st.rt_raw[2]), bits(m.rt_raw[3]))
    m.rtk = m.rtk.requires_grad_(True)                                   # rtk / rt_raw are detached as the reference does ...
    FS.save_latest_vars(m)
    m.kaug = m.kaug.requires_grad_(True)                                 # ... anything else that requires grad is refused
    with pytest.raises(NotImplementedError, match="require grad"):
        FS.save_latest_vars(m)


def test_reset_near_far_equals_get_near_far_after_a_hand_patch():
    name = "mixed/8"
    rtk, idk, nf0, rtk_all = G[name + "/rtk"], G[name + "/idk"], G[name + "/nf0"], G[name + "/rtk_all"]
    bounds = G["box/bounds"]
    mesh = types.SimpleNamespace(bounds=bounds.astype(np.float64), vertices=np.zeros((200, 3)))
    st = FS.FrameState.from_vars({"rtk": rtk, "idk": idk, "mesh_rest": mesh}, T(nf0).clone(), DEV)
    model = types.SimpleNamespace(latest_vars=st, near_far=st.near_far)
    FS.reset_near_far(model, T(rtk_all))
    hand = fn.patch_poses(rtk, idk, rtk_all).astype(np.float32)
    assert np.array_equal(bits(st.rtk), bits(hand))
    assert np.array_equal(bits(st.rtk[:, 3]), bits(rtk[:, 3]))           # row 3 survives the patch
    want, _ = run(fn.box_corners(bounds), hand, idk, nf0)                # explicit corners, table patched by hand, no rtk_all
    assert np.array_equal(bits(st.near_far), bits(want))
    with pytest.raises(NotImplementedError, match="require grad"):
        FS.reset_near_far(model, T(rtk_all).requires_grad_(True))
    st.mesh_rest = types.SimpleNamespace(bounds=None, vertices=np.zeros((0, 3)))
    with pytest.raises(ValueError, match="empty"):
        FS.reset_near_far(model, T(rtk_all))
    # a dict of numpy arrays, as scripts/visualize/nvs.py passes it, and a Parameter for a table
    nf = torch.nn.Parameter(T(nf0).clone())
    out = FS.get_near_far(nf, {"rtk": hand, "idk": idk}, pts=fn.box_corners(bounds))
    assert out is nf and np.array_equal(bits(nf.data), bits(want))


def test_frame_state_round_trip_and_the_latest_vars_view():
    rng = np.random.default_rng(3)
    v = {"rtk": rng.standard_normal((6, 4, 4)).astype(np.float32).astype(np.float64), "rt_raw": rng.standard_normal((6, 3, 4)).astype(np.float32),
         "idk": np.asarray([0, 1, 1, 0, 1, 0], np.float64), "obj_bound": np.asarray([0.3, 0.2, 0.25]), "mesh_rest": object(),
         "sil_err": np.arange(4.0)}
    st = FS.FrameState.from_vars(v, None, DEV)
    back = st.as_vars()
    assert set(back) == set(v)
    for k in ("rtk", "rt_raw", "idk", "obj_bound", "sil_err"):
        assert back[k].dtype == v[k].dtype and np.array_equal(back[k], v[k]), k
    assert back["mesh_rest"] is v["mesh_rest"]
    again = FS.FrameState.from_vars(back, None, DEV)
    assert all(np.array_equal(bits(getattr(again, k)), bits(getattr(st, k))) for k in ("rtk", "rt_raw", "idk"))
    # what mesh.extract_mesh (latest_vars['idk'].sum(), ['obj_bound']) and feeders.reinit_bones read
    assert float(st["idk"].sum()) == 3.0 and np.array_equal(np.asarray(st["obj_bound"], np.float32), np.float32([0.3, 0.2, 0.25]))
    assert "obj_bound" in st and "rtk" in st and "vis" not in st
    c = st["rtk"]
    c[:] = 0                                                             # a copy: the device table is untouched
    assert np.array_equal(st["rtk"], v["rtk"])
    with pytest.raises(ValueError, match="shape"):
        st["idk"] = np.zeros(5)
    empty = FS.FrameState(4, DEV)
    assert "obj_bound" not in empty and "mesh_rest" not in empty
    mesh = types.SimpleNamespace(vertices=np.asarray([[0.1, -0.5, 0.2]] * 101))
    assert np.allclose(FS.reset_obj_bound(empty, mesh), [0.12, 0.6, 0.24])
    assert float(FS.near_far_to_bound(T(G["box/nf32"]))) == pytest.approx(float(G["bound32"]), rel=1e-6)


def test_reset_nf():
    M = 16
    st = FS.FrameState(M, DEV)
    st.rtk.copy_(T(G["box/rtk"]))
    st.idk.fill_(1)
    verts = T(G["grid/pts"][:5004])
    model = types.SimpleNamespace(latest_vars=st, near_far=torch.nn.Parameter(torch.zeros(M, 2, device=DEV)), dp_verts_unit=verts, obj_scale=2.0)
    model.near_far.data[:, 1] = 6.0                                      # mean 3: shape_verts = verts / 3 * 3 * 1.2
    opts = types.SimpleNamespace(model_path="", bound_factor=2.0)
    FS.reset_nf(model, opts)
    sv = G["grid/pts"][:5004].astype(np.float32) / np.float32(3) * np.float32(3) * np.float32(1.2) * np.float32(2.0)
    assert np.allclose(st["obj_bound"], np.abs(sv).max(0), rtol=1e-6)
    want, bound = fn.get_near_far(np.zeros((M, 2)), G["box/rtk"], np.ones(M), sv)
    assert close(model.near_far.data.cpu().numpy(), want, bound + 4 * fn.U * np.abs(want)) <= 0     # (sv's own three roundings)
    kept = model.near_far.data.clone()
    FS.reset_nf(model, opts)                                             # planes are loaded now: they stay
    assert torch.equal(kept, model.near_far.data)


def test_captured_chain_follows_the_root_poses():
    """compute_rts -> reset_near_far -> raycast(..., near_far[fid]) in one graph at M = 8 and 16 rays: a replay after an in-place
    change of the root-pose parameters equals the eager result on the new parameters bit for bit, and differs from before."""
    from moda_amd import bench_support as BS
    from moda_amd.root_pose import compute_rts
    M = 8
    root = BS.make_root_rts(M, (0, M)).to(DEV).eval()
    from moda_amd import synth
    v, f = synth.make_rest_mesh()
    st = FS.FrameState(M, DEV)
    st.mesh_rest = moda_amd.TriMesh(T(v), T(f, torch.int32))
    st.idk.fill_(1)
    st.box()
    model = types.SimpleNamespace(latest_vars=st, near_far=st.near_far)
    rng = np.random.default_rng(11)
    xys = T(rng.uniform(0, 512, (M, 2, 2)).astype(np.float32))
    Kinv = T(np.tile(np.asarray([[1 / 400., 0, -0.64], [0, 1 / 400., -0.64], [0, 0, 1]], np.float32), (M, 1, 1)))
    fid = torch.arange(M, device=DEV)

    def chain():
        with torch.no_grad():
            rtk_all = compute_rts(root, M)
            nf = FS.reset_near_far(model, rtk_all)
            rays = moda_amd.raycast(xys, rtk_all[:, :3, :3], rtk_all[:, :3, 3], Kinv, nf[fid])
        return [rays[k] for k in ("near", "far", "rays_o", "rays_d")] + [nf]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            first = [t.clone() for t in chain()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, outs))
    with torch.no_grad():
        root.base_rt.se3.add_(T(rng.standard_normal(tuple(root.base_rt.se3.shape)).astype(np.float32)) * 0.05)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in outs]
    eager = [t.clone() for t in chain()]
    torch.cuda.synchronize()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(replayed, eager))
    assert not torch.equal(replayed[-1], first[-1]) and not torch.equal(replayed[1], first[1])      # the table and the rays' far plane
    # (the near plane of this box, 0.3 in front of the camera, is the 1e-3 clamp before and after)
    assert torch.isfinite(replayed[-1]).all() and (replayed[-1][:, 1] > replayed[-1][:, 0]).all()
    st.check()


def test_harness_nf_reset():
    """TrainHarness(nf_reset=True): the eager and the replayed step leave the same near_far table bit for bit.  Harness A runs two
    eager steps, harness B one eager warm-up step and two replays, from the same seeds: A's first table equals B's warm-up table
    and A's second equals B's first replay -- both follow from the initial parameters and from AdamW's first update, whose
    m / (sqrt(v) + eps) = g / (|g| + eps) does not feel the last bits of a gradient.  The table of B's second replay is held bit
    for bit to an eager get_near_far over the pose table that replay itself patched: a cross-harness comparison there would
    hang on the root MLP's bias gradients, which the column sum adds with float atomics."""
    from moda_amd import bench_support as BS
    kw = dict(N=256, S=16, default_losses=True, root_pose=True)
    with pytest.raises(ValueError, match="root_pose"):
        BS.TrainHarness(N=256, S=16, default_losses=True, nf_reset=True)
    off = BS.TrainHarness(**kw)
    assert off.frames is None and off.near_far is None and not hasattr(off, "latest_vars")
    a = BS.TrainHarness(nf_reset=True, **kw)
    a.eager_step()
    a1 = a.near_far.clone()
    a.eager_step()
    a2 = a.near_far.clone()
    b = BS.TrainHarness(nf_reset=True, **kw)
    b.capture(warm=1)
    b0 = b.near_far.clone()
    b.step()
    b1 = b.near_far.clone()
    b.step()
    torch.cuda.synchronize()
    b2 = b.near_far.clone()
    assert np.array_equal(bits(a1), bits(b0)) and np.array_equal(bits(a2), bits(b1))
    assert not np.array_equal(bits(a1), bits(a2)) and not np.array_equal(bits(b1), bits(b2))
    nf = torch.zeros_like(b2)
    FS.get_near_far(nf, b.frames)                                        # the patched table, the same box, no rtk_all
    assert np.array_equal(bits(nf), bits(b2))
    assert torch.isfinite(b2).all() and (b2[:, 1] > b2[:, 0]).all() and b.frames.status.cpu().tolist() == [0, 0, 0, 0]
    assert np.array_equal(b.frames["idk"], np.ones(b.n_frames, np.float32))
