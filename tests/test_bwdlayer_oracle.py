"""CPU: the references, bounds and kernel models of tests/bwdlayer_numpy.py, which tests/test_gpu_bwdlayer.py holds the bf16-storage
backward kernels to.
  * the closed forms equal float64 torch autograd (one Linear + ReLU per link, the bf16 rounding between links applied by hand;
    Embedding's backward through oracle/torch_ref.py's restatement);
  * every exact-kind case of the GPU file's lists meets its exactness conditions (asserted inside the references: integer truths,
    |baseline| + sum |term| < 2^24 units, bf16-stored values integers <= 256, the bound of an element a subnormal reaches < 1),
    and a dropped row or tile shows inside those elements at the largest M;
  * an fp32 numpy model that sums tile by tile in each kernel's order reproduces the exact kind bit for bit and stays inside the
    random kind's bars;
  * the same model with one planted fault is caught by the exact-kind cases and outputs CATCH lists for that fault;
  * tests/dev_entries.py parses moda_dev.h and, where the library is built, finds each entry's one mangled name in its ELF."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import bwdlayer_numpy as B
import dev_entries

F64 = torch.float64


# ---- dev_entries -----------------------------------------------------------------------------------------------------------------
def test_dev_entries_reads_the_declarations():
    sig = dev_entries.signatures()
    assert tuple(sig) == dev_entries.ENTRIES
    P, LL, I, TAB, LLTAB = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_longlong)
    assert sig["moda_chain64_part_floats"] == (LL, [LL])
    assert sig["moda_bwd256_layer"] == (I, [I, P, LL, P, LL, P, LL, P, LL, P, LL, P, LL, P])
    assert sig["moda_chain64_bwd"] == (I, [P, LL, TAB, LL, TAB, P, LL, TAB, LLTAB, TAB, I, LL, P, P])
    assert sig["moda_heads64_bwd"] == (I, [P, LL, P, LL, P, LL, P, P, P, LL, P, LL, P, I, P, P, LL, P, P])
    assert sig["moda_pe_ends64_bwd"] == (I, [P, P, LL, P, LL, P, P, P, I, P, P, LL, P, LL, P, P, LL, P, P])


def test_dev_entries_parameter_types_with_and_without_names():
    assert dev_entries.parameter_type("long long") == dev_entries.parameter_type("long long M") == "long long"
    assert dev_entries.parameter_type("const void* const* h") == dev_entries.parameter_type("const void *const *") == "const void* const*"
    assert dev_entries.parameter_type("float* part") == "float*"
    with pytest.raises(AssertionError):
        dev_entries.parameter_type("size_t n")                    # a type this parser does not know is an error, not a guess


def test_dev_entries_finds_each_entry_once_in_the_built_library():
    from moda_amd.build import LIB_PATH
    if not os.path.exists(LIB_PATH):
        pytest.skip("libmoda_hip.so is not built")
    names = dev_entries.dynamic_symbols(LIB_PATH)
    assert "moda_abi_version" in names and "moda_gemm_f32_ex" in names
    for ident in dev_entries.ENTRIES:
        assert dev_entries.mangled(names, ident).startswith(f"_Z{len(ident)}{ident}")
    with pytest.raises(AssertionError):
        dev_entries.mangled(names, "moda_chain64")                # a prefix of two entries' names is no match: the length differs
    fns = dev_entries.bind(ctypes.CDLL(LIB_PATH), LIB_PATH)
    assert fns["moda_chain64_part_floats"](65665) == 512 * 4 * (64 * 64 + 64)      # host arithmetic: runs without a GPU
    assert fns["moda_chain64_part_floats"](129) == 2 * 4 * (64 * 64 + 64)


# ---- the closed forms against float64 autograd -------------------------------------------------------------------------------------
def autograd_layer(dz, x, w):
    """dW, db and d(pre-activation) of sum(dZ . (relu(P) W^T + b)) at P = x."""
    P = torch.tensor(x, dtype=F64, requires_grad=True)
    Wt = torch.tensor(w, dtype=F64, requires_grad=True)
    b = torch.zeros(w.shape[0], dtype=F64, requires_grad=True)
    (torch.tensor(dz, dtype=F64) * (torch.relu(P) @ Wt.T + b)).sum().backward()
    return Wt.grad.numpy(), b.grad.numpy(), P.grad.numpy()


def close(a, b):
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kind", B.KINDS)
def test_layer_reference_equals_float64_autograd(kind):
    c = B.make_layer(kind, "sparse", 37, 128)
    ref = B.ref_layer(c)
    dW, db, dP = autograd_layer(B.bf16_val(c["dz"]), B.bf16_val(c["x"]), B.bf16_val(c["w"]))
    close(ref["gW"][0], c["gW0"] + dW)
    close(ref["gb"][0], c["gb0"] + db)
    close(ref["dX"][0], dP)
    x = B.bf16_val(c["x"])
    special = np.isin(c["x"], B.SPECIALS)
    assert special.any() and (ref["dX"][0][special & (x <= 0)] == 0).all()
    assert (ref["dX"][0][c["x"] == 0x0001] != 0).any()               # the positive subnormal passes


@pytest.mark.parametrize("kind", B.KINDS)
def test_chain_references_equal_float64_autograd_link_by_link(kind):
    c = B.make_chain(kind, "sparse", 131)
    ref = B.ref_chain(c)
    dh = B.bf16_val(c["dh"])
    for l in range(4):
        dW, db, dP = autograd_layer(dh, B.bf16_val(c["h"][l]), B.bf16_val(c["w"][l]))
        close(ref[f"gW{l}"][0], c["gW0"][l] + dW)
        close(ref[f"gb{l}"][0], c["gb0"][l] + db)
        close(ref[f"dX{l}"][0], dP)
        dh = torch.tensor(dP).bfloat16().double().numpy()             # dh rounded to bf16 between layers, db from the rounded values
    h = B.make_heads(kind, "sparse", 131, 25)
    ref = B.ref_heads(h)
    dW, db, dP = autograd_layer(B.bf16_val(h["dz"]), B.bf16_val(h["dd"]), B.bf16_val(h["wrgb"]))
    close(ref["g_rgb"][0], h["g_rgb0"] + dW)
    close(ref["g_brgb"][0], h["g_brgb0"] + db)
    dzd = torch.tensor(dP).bfloat16().double().numpy()
    dW, db, dP = autograd_layer(dzd, B.bf16_val(h["hD"]), B.bf16_val(h["wext"]))
    close(ref["Tm"][0], h["Tm0"] + dW)
    close(ref["svec"][0], h["svec0"] + db)
    close(ref["dh"][0], dP)


@pytest.mark.parametrize("n_freq,alpha", [(10, 6.3), (6, 3.4), (10, 10.0)])
def test_embedding_backward_equals_float64_autograd_of_the_restatement(n_freq, alpha):
    import math
    from oracle import torch_ref
    rng = np.random.default_rng(3)
    x = torch.tensor(rng.standard_normal((50, 3)) * 1.5, dtype=F64, requires_grad=True)
    g = rng.standard_normal((50, 3 + 6 * n_freq))
    (torch.tensor(g) * torch_ref.embedding(x, n_freq, alpha)).sum().backward()
    win = np.array([0.5 * (1 + math.cos(math.pi * min(max(alpha - k, 0.0), 1.0) + math.pi)) for k in range(n_freq)])
    close(B.embed_backward(g, x.detach().numpy(), win), x.grad.numpy())
    assert np.array_equal(B.window(n_freq, alpha), win.astype(np.float32))
    c = B.make_pe("random", 50, n_freq, alpha)
    dpe = B.bf16_val(c["dha"]) @ B.bf16_val(c["wa"]) + B.bf16_val(c["dhb"]) @ B.bf16_val(c["wb"])
    close(B.ref_pe(c)["d_xyz"][0], B.embed_backward(dpe, c["xyz"].astype(np.float64), c["win"].astype(np.float64)))


# ---- the exactness conditions of every case of the GPU file ------------------------------------------------------------------------
@pytest.mark.parametrize("entry,variant", [(e, v) for e in ("bwd256", "chain64", "heads64", "signmap") for v in ("sparse", "onehot")]
                         + [("pe_ends64", "dense")])
def test_exact_kind_cases_meet_their_exactness_conditions(entry, variant):
    """The references assert the conditions (assert_exact); here every case of the GPU file's lists is built and referenced."""
    if entry == "bwd256":
        for W, Ms in ((256, B.M_256), (128, B.M_128)):
            for M in Ms:
                B.ref_layer(B.make_layer("exact", variant, M, W))
    elif entry == "chain64":
        for M in B.M_CHAIN:
            B.ref_chain(B.make_chain("exact", variant, M))
    elif entry == "heads64":
        for M in B.M_HEADS:
            for n_out in B.N_OUT:
                B.ref_heads(B.make_heads("exact", variant, M, n_out))
    elif entry == "pe_ends64":
        for M in B.M_HEADS:
            for n_freq, alpha in B.PE_WINDOWS:
                B.ref_pe(B.make_pe("exact", M, n_freq, alpha))
    else:
        for K in B.K_MAPS:
            for R, N in B.RN_MAPS:
                B.ref_layer(B.make_rect("exact", variant, K, R, N))


# ---- the fp32 tile-order models: inside the bars, exact on the exact kind, and failing with a planted fault --------------------------
@functools.lru_cache(maxsize=None)
def case(entry, kind, *args):
    if entry == "bwd256":
        c = B.make_layer(kind, "sparse", args[1], args[0])
        return c, B.ref_layer(c), B.model_bwd256
    if entry == "chain64":
        c = B.make_chain(kind, "sparse", *args)
        return c, B.ref_chain(c), B.model_chain
    if entry == "heads64":
        c = B.make_heads(kind, "sparse", *args)
        return c, B.ref_heads(c), B.model_heads
    c = B.make_pe(kind, *args)
    return c, B.ref_pe(c), B.model_pe_ends


MODEL_CASES = ([("bwd256", 256, M) for M in (1, 33, 65, 576, 8257)] + [("bwd256", 128, M) for M in (33, 65, 16449)]
               + [("chain64", M) for M in (1, 33, 129, 513, 893)] + [("heads64", 33, 16), ("heads64", 513, 25), ("heads64", 893, 1)]
               + [("pe_ends64", 33, 10, 6.3), ("pe_ends64", 513, 6, 3.4), ("pe_ends64", 893, 10, 6.3)])


@pytest.mark.parametrize("spec", MODEL_CASES, ids=lambda s: "-".join(str(v) for v in s))
def test_tile_order_model_is_exact_on_the_exact_kind_and_inside_the_random_bars(spec):
    for kind in B.KINDS:
        c, ref, model = case(spec[0], kind, *spec[1:])
        res = B.compare(ref, model(c), f"{spec} {kind}")
        assert all(ok for _, ok in res.values()), res


CHAIN_G = tuple(f"g{t}{l}" for t in "Wb" for l in range(4))
CATCH = {       # fault -> [(entry and arguments of an exact-kind case, the kernel outputs that differ)]
    "short_row": [(("bwd256", 256, 33), ("dX", "gW", "gb")), (("bwd256", 128, 65), ("dX", "gW", "gb")), (("chain64", 129), CHAIN_G + ("dh",)),
                  (("heads64", 513, 25), ("g_rgb", "g_brgb", "Tm", "svec", "dh")), (("pe_ends64", 893, 10, 6.3), ("gWa", "gWb", "gb_b", "d_xyz"))],
    "skip_ring_tile": [(("bwd256", 256, 24641), ("dX", "gW", "gb")), (("bwd256", 128, 65601), ("dX", "gW", "gb"))],
    "db_half": [(("bwd256", 256, 33), ("gb",)), (("bwd256", 128, 65), ("gb",)), (("chain64", 129), CHAIN_G[4:]),
                (("heads64", 513, 25), ("g_brgb", "svec")), (("pe_ends64", 513, 6, 3.4), ("gb_b",))],
    "no_remainder": [(("chain64", 513), CHAIN_G), (("chain64", 893), CHAIN_G), (("heads64", 893, 1), ("g_rgb", "g_brgb", "Tm", "svec")),
                     (("pe_ends64", 513, 6, 3.4), ("gWa", "gWb", "gb_b"))],
    "mask_ge": [(("bwd256", 256, 1), ("dX",)), (("bwd256", 128, 33), ("dX",)), (("chain64", 33), ("dh", "gW1", "gb3")),
                (("heads64", 33, 16), ("dh", "Tm", "svec"))],
    "mask_neighbour": [(("bwd256", 256, 33), ("dX",)), (("bwd256", 128, 65), ("dX",)), (("chain64", 33), ("dh", "gW1", "gb3"))],
    "flush_subnormal": [(("bwd256", 256, 1), ("dX",)), (("bwd256", 128, 33), ("dX",)), (("chain64", 33), ("dh", "gW1", "gb3")),
                        (("heads64", 33, 16), ("dh", "Tm", "svec"))],
}


@pytest.mark.parametrize("fault", list(CATCH))
def test_planted_fault_is_caught_by_its_exact_kind_cases(fault):
    for spec, outputs in CATCH[fault]:
        c, ref, model = case(spec[0], "exact", *spec[1:])
        res = B.compare(ref, model(c, fault), f"{fault} {spec}", show=False)
        caught = {k for k, (_, ok) in res.items() if not ok}
        assert set(outputs) <= caught, (fault, spec, sorted(caught))


@pytest.mark.parametrize("W,M", [(256, 24641), (128, 65601)])
@pytest.mark.parametrize("fault", ["short_row", "skip_ring_tile"])
def test_dropped_rows_show_inside_the_columns_a_subnormal_reaches(fault, W, M):
    """The elements of gW that carry a bound in the exact kind (a subnormal of X reaches them) see a dropped tail row and a
    dropped tile as well as the bit-exact ones do: the bound stays below 1 at the largest M, the fault moves integers by >= 2."""
    c, ref, model = case("bwd256", "exact", W, M)
    truth, bound = ref["gW"]
    barred = bound > 0
    assert 0.15 < barred.mean() < 0.30 and bound.max() < 0.5
    clean, bad = model(c)["gW"], model(c, fault)["gW"]
    assert (np.abs(clean - truth) <= bound).all()
    moved = bad != clean
    assert (moved & barred).any()
    assert (np.abs(bad - truth)[moved] > bound[moved]).all() and (np.abs(bad - clean)[moved] >= 2).all()
    res = B.compare({"gW": (truth[:, barred.any(0)], bound[:, barred.any(0)])}, {"gW": bad[:, barred.any(0)]}, show=False)
    assert not res["gW"][1]


@pytest.mark.parametrize("K", [1, 127, 129, 8257])
def test_sign_map_model_and_its_planted_fault(K):
    """model_signmap equals [B > 0] bit for bit with the bytes around it untouched; with the bits of the ragged last k-tile taken
    from the wrong rows it differs on every ragged K of the GPU test."""
    for variant in ("sparse", "onehot"):
        x = B.make_rect("exact", variant, K, 64, 64)["x"]
        want = B.ref_signmap(x)
        got = B.model_signmap(x, 11)
        assert np.array_equal(got[:, :8], want) and (got[:, 8:] == 0xAA).all()
        assert (B.model_signmap(x, 11, "bits_wrong_rows")[:, :8] != want).any()
    s = np.array([[0x0000, 0x8000, 0x0001, 0x8001, 0x3F80, 0xBF80, 0x7F80, 0xFF80]], np.uint16)
    assert B.ref_signmap(s)[0, 0] == 0b01010100 == B.model_signmap(s, 1)[0, 0]


def test_every_fault_has_a_catching_case():
    assert set(CATCH) | {"bits_wrong_rows"} == set(B.FAULTS)
