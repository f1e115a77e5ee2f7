"""CPU: the float64 oracle of gradient clipping (tests/clip_numpy.py) against torch.nn.utils.clip_grad_norm_ -- the function
the reference's clip_grad calls (nnutils/train_utils.py:1285-1306) -- the name -> group chain of moda_amd.train_utils against a
hand-written list, and the conditions tests/test_gpu_clip_grad.py relies on, for the cases both files share.

Bar of (a), u = 2^-24: clip_grad_norm_ sums n non-negative fp32 squares in fp32 in an order of its own; for ANY order the sum is
within (n - 1) u relative, each square adds 1 u, the square root halves the total and adds 1 u, the norm of the per-tensor norms
repeats that for a handful of terms: a group norm of n elements is within (n / 2 + 8) u of the float64 one, its coefficient 3 u
further (add, divide, the fp32 threshold is shared), a scaled gradient one more."""
import numpy as np
import pytest
import torch

import clip_numpy as cn
from moda_amd import train_utils as TU

U = 2.0 ** -24
CHUNK = 4096
CLIP_SCALE = 1.0
# (name, numel, standard deviation of the gradient, flag); parameter order matters: nerf_coarse and nerf_skin interleave
TENSORS = (
    ("nerf_coarse.xyz_encoding_1.0.weight", 2 * CHUNK + 3, 0.02, None),
    ("nerf_skin.xyz_encoding_1.0.weight", CHUNK + 1, 0.0005, None),
    ("nerf_coarse.xyz_encoding_1.0.bias", CHUNK, 0.02, None),
    ("nerf_skin.xyz_encoding_1.0.bias", 5, 0.0005, None),
    ("nerf_coarse.beta", 1, 0.3, None),
    ("nerf_feat.rgb.0.weight", 3, 1.0, None),
    ("nerf_feat.beta", 1, 0.01, None),
    ("nerf_vis.rgb.0.weight", 4, 0.5, None),
    ("rest_pose_code.weight", CHUNK + 1, 2.0, "misaligned"),      # its .grad starts 4 bytes off 16-byte alignment
    ("bones", CHUNK, 0.1, None),
    ("skin_aux", 3, 0.01, None),
    ("nerf_body_rts.1.weight", 7, 0.0, "no_grad"),                # .grad is None
    ("mystery.weight", CHUNK + 1, 0.25, None),                    # matches no group: scanned, never scaled
    ("module.nerf_unc.rgb.0.bias", 5, 1.0, None),
)
NAMES = [t[0] for t in TENSORS]
GROUPS = [TU.grad_group(n) for n in NAMES]
FACTORS = [f for _, f in TU.GRAD_GROUPS]
MAX_NORM = np.asarray([f * CLIP_SCALE for f in FACTORS], np.float64).astype(np.float32)
GPU_CASES = {
    "vis_frozen": dict(seed=1, frozen=("nerf_vis",)),
    "shape_frozen": dict(seed=2, frozen=("nerf_coarse", "nerf_beta", "nerf_vis", "bones", "pose_code")),
}
# one non-finite value: (tensor index, element index)
POISON_AT = {"tail": (0, 2 * CHUNK + 2), "frozen": (7, 2), "ungrouped": (12, CHUNK)}
POISON_KIND = {"nan": np.float32(np.nan), "inf": np.float32(np.inf)}


def make_grads(seed):
    rng = np.random.default_rng(seed)
    return [None if flag == "no_grad" else (rng.standard_normal(n) * s).astype(np.float32) for _, n, s, flag in TENSORS]


def frozen_ids(case):
    return {TU.GROUP_INDEX[g] for g in case["frozen"]}


def oracle(case, poison=None):
    grads = make_grads(case["seed"])
    if poison is not None:
        kind, where = poison
        t, e = POISON_AT[where]
        grads[t][e] = POISON_KIND[kind]
    return grads, cn.clip_grad_f64(grads, GROUPS, MAX_NORM, frozen_groups=frozen_ids(case))


def cpu_params(grads):
    out = []
    for name, g in zip(NAMES, grads):
        p = torch.nn.Parameter(torch.zeros(1 if g is None else g.size))
        if g is not None:
            p.grad = torch.from_numpy(g.copy())
        out.append((name, p))
    return out


@pytest.mark.parametrize("case", sorted(GPU_CASES))
def test_oracle_agrees_with_clip_grad_norm(case):
    c = GPU_CASES[case]
    grads, ref = oracle(c)
    named = cpu_params(grads)
    norms, invalid = cn.clip_grad_torch(named, TU.grad_group, FACTORS, CLIP_SCALE, frozen_groups=frozen_ids(c))
    assert not invalid and not ref["invalid"]
    count = np.zeros(len(FACTORS))
    for g, gi in zip(grads, GROUPS):
        if g is not None and gi is not None:
            count[gi] += g.size
    for gi, n in enumerate(norms):
        bar = (count[gi] / 2 + 8) * U
        err = abs(float(n) - ref["norms"][gi]) / max(ref["norms"][gi], 1e-300) if ref["norms"][gi] else abs(float(n))
        print(TU.GRAD_GROUPS[gi][0], "norm", ref["norms"][gi], "err / u", err / U, "bar / u", bar / U)
        assert err <= bar
    for (name, p), r, gi in zip(named, ref["grads"], GROUPS):
        if r is None:
            assert p.grad is None
            continue
        got = p.grad.numpy().astype(np.float64)
        bar = ((count[gi] / 2 + 12) * U) if gi is not None else 0.0
        assert (np.abs(got - r) <= bar * np.abs(r)).all(), name


def test_oracle_nan_zeroes_everything_like_the_reference():
    c = GPU_CASES["vis_frozen"]
    grads = make_grads(c["seed"])
    grads[7][2] = np.nan                                     # inside the frozen group: tested before the freeze
    ref = cn.clip_grad_f64(grads, GROUPS, MAX_NORM, frozen_groups=frozen_ids(c), reject_inf=False)
    named = cpu_params(grads)
    _, invalid = cn.clip_grad_torch(named, TU.grad_group, FACTORS, CLIP_SCALE, frozen_groups=frozen_ids(c))
    assert invalid and ref["invalid"] and ref["n_nan"] == 1
    for (_, p), r in zip(named, ref["grads"]):
        if r is not None:
            assert float(p.grad.abs().max()) == 0.0 and float(np.abs(r).max()) == 0.0


def test_grad_group_names():
    gi = TU.GROUP_INDEX
    assert [n for n, _ in TU.GRAD_GROUPS] == [
        "nerf_coarse", "nerf_beta", "nerf_feat", "nerf_beta_feat", "nerf_fine", "nerf_unc", "nerf_flowbw", "nerf_skin", "nerf_dis",
        "nerf_vis", "nerf_root_rts", "nerf_body_rts", "root_code", "pose_code", "env_code", "appearance_code", "vid_code", "bones",
        "skin_aux", "ks", "nerf_dp", "csenet"]
    assert FACTORS == [1, 1, .1, .1, .1, .1, .1, .1, .1, .1, 100, 100, .1, 100, .1, .1, .1, 1, .1, .1, .1, .1]
    expect = {
        "nerf_coarse.xyz_encoding_1.0.weight": "nerf_coarse",
        "nerf_coarse.beta": "nerf_beta",                         # beta splits off from nerf_coarse ...
        "nerf_feat.sigma.0.bias": "nerf_feat",
        "nerf_feat.beta": "nerf_beta_feat",                      # ... and from nerf_feat
        "nerf_fine.dir_encoding.0.weight": "nerf_fine",
        "nerf_unc.rgb.0.weight": "nerf_unc",
        "nerf_flowbw.xyz_encoding_1.0.weight": "nerf_flowbw",
        "nerf_flowfw.xyz_encoding_1.0.weight": "nerf_flowbw",
        "nerf_skin.rgb.0.weight": "nerf_skin",
        "nerf_dis.rgb.0.weight": "nerf_dis",
        "nerf_vis.rgb.0.weight": "nerf_vis",
        "nerf_root_rts.0.weight": "nerf_root_rts",
        "nerf_root_rts.root_code.weight": "nerf_root_rts",       # the network test comes before the code test
        "nerf_body_rts.0.weight": "nerf_body_rts",
        "nerf_body_rts.1.bones": "nerf_body_rts",                # `bones` inside another name is not the bones group
        "nerf_body_rts.0.pose_code.weight": "nerf_body_rts",
        "root_code.weight": "root_code",
        "pose_code.weight": "pose_code",
        "rest_pose_code.weight": "pose_code",
        "env_code.weight": "env_code",
        "appearance_code.weight": "appearance_code",
        "vid_code.weight": "vid_code",
        "bones": "bones",
        "skin_aux": "skin_aux",
        "ks_param": "ks",
        "nerf_dp.rgb.0.weight": "nerf_dp",
        "csenet.net.0.weight": "csenet",
        "nerf_dp.csenet.weight": "nerf_dp",                      # order of the last two tests
        "nerf_skin.beta": "nerf_skin",                           # beta splits only coarse and feat
        "nerf_coarse.nerf_feat.beta": "nerf_beta",               # first match wins
        # whole names only
        "bones_rst": None, "bones.weight": None, "my_bones": None, "skin_aux.0": None, "ks_param.weight": None, "ks": None,
        # nothing matches
        "near_far": None, "mystery.weight": None, "nerf_coars.weight": None, "": None,
    }
    for name, g in expect.items():
        want = None if g is None else gi[g]
        assert TU.grad_group(name) == want, name
        assert TU.grad_group("module." + name) == want, "module." + name
    assert TU.grad_group("module.module.bones") is None          # one prefix is stripped, as DistributedDataParallel adds one


def test_chunk_table_layout():
    segs = [(g.size, -1 if gi is None else gi) for g, gi in zip(make_grads(1), GROUPS) if g is not None]
    chunk_seg, chunk_off, group_begin = TU.build_tables(segs)
    assert len(group_begin) == len(FACTORS) + 1 and group_begin[0] == 0
    assert len(chunk_seg) == sum(-(-n // CHUNK) for n, _ in segs)
    seen = [[] for _ in segs]
    for c, (s, off) in enumerate(zip(chunk_seg, chunk_off)):
        assert off % CHUNK == 0 and 0 <= off < segs[s][0]
        seen[s].append(off)
        g = segs[s][1]
        lo, hi = (group_begin[g], group_begin[g + 1]) if g >= 0 else (group_begin[-1], len(chunk_seg))
        assert lo <= c < hi
    for s, (n, _) in enumerate(segs):
        assert seen[s] == list(range(0, n, CHUNK))
    # nerf_coarse's two tensors are not neighbours in parameter order, its chunks are
    coarse = TU.GROUP_INDEX["nerf_coarse"]
    assert [chunk_seg[c] for c in range(group_begin[coarse], group_begin[coarse + 1])] == [0, 0, 0, 2]


@pytest.mark.parametrize("case", sorted(GPU_CASES))
def test_gpu_cases_are_clear_of_the_clamp_threshold(case):
    _, ref = oracle(GPU_CASES[case])
    for gi, (norm, mx) in enumerate(zip(ref["norms"], MAX_NORM.astype(np.float64))):
        assert abs(norm + 1e-6 - mx) > 1e-3 * mx, (TU.GRAD_GROUPS[gi][0], norm, mx)


def test_gpu_cases_cover_every_kind_of_group():
    kinds = set()
    for c in GPU_CASES.values():
        grads, ref = oracle(c)
        present = {gi for g, gi in zip(grads, GROUPS) if g is not None and gi is not None}
        for gi in range(len(FACTORS)):
            if gi in frozen_ids(c):
                assert gi in present and ref["norms"][gi] == 0.0
                kinds.add("frozen")
            elif gi not in present:
                assert ref["norms"][gi] == 0.0
                kinds.add("empty")
            else:
                kinds.add("clamped" if ref["coef"][gi] < 1.0 else "unclamped")
    assert kinds == {"frozen", "empty", "clamped", "unclamped"}
    assert any(gi is None for gi in GROUPS) and GROUPS[TENSORS.index(TENSORS[11])] == TU.GROUP_INDEX["nerf_body_rts"]
