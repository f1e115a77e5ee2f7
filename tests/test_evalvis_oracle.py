"""CPU: the float64 restatement tests/evalvis_numpy.py against the reference's own flow_to_image, make_color_wheel and image_grid
(tests/golden/g39_evalvis.npz, tests/golden/gen_golden_evalvis.py), the nearest resize against torch on the CPU, and the second
ABI header.  The eval() canvas block and save_vid are restated, not pinned (methods behind heavy imports)."""
import importlib
import os

import numpy as np
import pytest
import torch

import evalvis_numpy as en

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "g39_evalvis.npz"))
CASES = ("rand64", "smooth64", "unknown33x31", "nan5x7", "zero5x7", "one1x1")


def test_wheel_is_the_references_and_the_modules_is_generated_equal():
    EF = importlib.import_module("moda_amd.eval_frames")
    assert G["wheel"].shape == (55, 3)
    assert np.array_equal(en.color_wheel(), G["wheel"]) and np.array_equal(EF.color_wheel(), G["wheel"])


@pytest.mark.parametrize("case", CASES)
def test_flow_to_image_restatement_equals_the_reference(case):
    """Both of the reference's runs, the fp32 input (float64 after the division under numpy >= 2, which generated the file)
    and the float64 input, bit for bit; the caller's array is not written."""
    assert int(str(G["numpy_version"]).split(".")[0]) >= 2
    flow = G[case + "/flow"]
    keep = flow.copy()
    assert np.array_equal(en.flow_to_image(flow)[0], G[case + "/img32"])
    assert np.array_equal(flow, keep, equal_nan=True)
    assert np.array_equal(en.flow_to_image(flow.astype(np.float64))[0], G[case + "/img64"])
    assert int((G[case + "/img32"] != G[case + "/img64"]).sum()) == int(G[case + "/ndiff"])


@pytest.mark.parametrize("case", CASES)
def test_flow_fp32_arithmetic_differs_only_where_the_rule_allows(case):
    """numpy < 2's arithmetic (fp32 after the division) against the golden: differences only on undecided channels (not exact by
    construction, 255 col within 0.01 of an integer) and on the pixels of maximal radius, where one of the two branch values."""
    img, pre, exact, top, alt = en.flow_to_image(G[case + "/flow"], np.float32)
    want = G[case + "/img32"]
    und = ~exact & (np.abs(pre - np.round(pre)) < 0.01) & ~top[..., None]
    d = img.astype(int) - want.astype(int)
    assert not (d != 0)[~und & ~top[..., None]].any() and np.abs(d[und]).max(initial=0) <= 1
    t = np.broadcast_to(top[..., None], img.shape)
    assert ((want[t] == img[t]) | (want[t] == alt[t])).all()


def test_image_grid_equals_the_reference():
    assert np.array_equal(en.image_grid(G["grid/img"], 3, 3), G["grid/out"])
    assert np.array_equal(en.image_grid(G["grid1/img"], 1, 1), G["grid1/out"])


@pytest.mark.parametrize("Sm,S", [(8, 8), (12, 8), (16, 8), (5, 8), (7, 64), (100, 64), (3, 1)])
def test_nearest_resize_is_torchs(Sm, S):
    m = np.random.default_rng(Sm * 100 + S).standard_normal((2, Sm, Sm)).astype(np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(m)[:, None], (S, S))[:, 0].numpy()
    assert np.array_equal(en.nearest_resize(m, S), want)


def test_to_u8_rule_equals_numpy_in_range():
    v = np.asarray([-0.5, 0.0, 0.999, 1.0, 127.5, 255.0, 255.9], np.float32)
    out, ns, nn = en.to_u8(v)
    assert np.array_equal(out, v.astype(np.uint8)) and (ns, nn) == (0, 0)
    out, ns, nn = en.to_u8(np.asarray([-1.0, 256.0, 1e9, -1e9, np.inf, np.nan], np.float32))
    assert out.tolist() == [0, 255, 255, 0, 255, 0] and (ns, nn) == (5, 1)


def test_second_header_parses_and_is_exported():
    from moda_amd import abi, build, _lib
    assert len(abi.PROTOTYPES) == 141 and not set(abi.PROTOTYPES) & set(abi.VIS_PROTOTYPES)
    names = ("moda_vis_minmax", "moda_vis_apply", "moda_flow_color", "moda_vis_grid", "moda_vis_to_u8")
    assert tuple(abi.VIS_PROTOTYPES) == names == _lib.VIS_EXPORTS
    assert all(k.startswith("MODA_VIS_") for k in abi.VIS_CONSTANTS) and not set(abi.VIS_CONSTANTS) & set(abi.CONSTANTS)
    assert abi.VIS_CONSTANTS["MODA_VIS_TILE"] % abi.VIS_CONSTANTS["MODA_VIS_BLOCK"] == 0
    assert "evalvis_kernels.hip" in build.SOURCES and any(h.endswith("moda_hip_vis.h") for h in build.HEADERS)
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert _lib._VIS_SIGNATURES["moda_vis_to_u8"][1][-1] is _lib._P


def test_package_exports_and_refusals_without_a_gpu():
    import moda_amd
    for name in ("nerf_render_eval", "render_vid", "eval_canvases", "flow_to_image", "image_grid", "to_display", "video_frames",
                 "eval_frames", "EvalFrames"):
        assert hasattr(moda_amd, name), name
    EF = importlib.import_module("moda_amd.eval_frames")
    with pytest.raises(RuntimeError, match="only compute path"):
        EF.flow_to_image(torch.zeros(1, 2, 2, 2))
    with pytest.raises(NotImplementedError, match="require grad"):
        EF.image_grid(torch.zeros(1, 2, 2, 2, requires_grad=True), 1, 1)
