"""CPU (no GPU needed): include/moda_hip.h is the only description of the C ABI.  moda_amd/abi.py parses it, moda_amd/_lib.py
derives every ctypes signature and descriptor struct from the parse, and the modules read their MODA_* constants from it.
Checked here: the parse is complete, a few signatures are pinned as literals (so an error in the type map cannot hide behind the
derivation), the structs have the layout the C++ compiler gives them, and the parser refuses what it does not understand."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from moda_amd import _lib, abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "moda_hip.h")
P, PP, I32, I64, F32, F64 = C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_float, C.c_double
STRUCTS = {"moda_mlp_desc": _lib.MlpDesc, "moda_gemm_desc": _lib.GemmDesc, "moda_nerf_train_desc": _lib.NerfTrainDesc,
           "moda_asm_term": _lib.AsmTerm}


@pytest.fixture(scope="module")
def header():
    return open(HEADER).read()


def test_every_prototype_struct_and_constant_of_the_header_is_parsed(header):
    build.build(verbose=False)
    lib = _lib.load()
    declared = set(re.findall(r"\b(moda_[a-z0-9_]+)\s*\(", header))          # test_host_cpu.py's independent regex
    assert set(abi.PROTOTYPES) == declared == set(_lib.EXPORTS)
    assert len(abi.PROTOTYPES) == 141
    for name in abi.PROTOTYPES:
        assert hasattr(lib, name), f"{name} is not a symbol of the built library"
    assert set(abi.STRUCTS) == set(STRUCTS)
    defines = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MODA_\w+)[ \t]+\(?(-?\d+)\)?", header, flags=re.M)}
    assert len(defines) > 60 and "MODA_HIP_H" not in abi.CONSTANTS
    assert abi.CONSTANTS == defines
    assert abi.CONSTANTS["MODA_EINVAL"] == -1 and abi.CONSTANTS["MODA_ESHAPE"] == -2


def test_pinned_signatures():
    """Literals from the hand-written table this derivation replaced (its POINTER(c_int64) host arrays are c_void_p now)."""
    sig = _lib._SIGNATURES
    assert sig["moda_mlp_fwd"] == (C.c_int, [C.POINTER(_lib.MlpDesc), P, P, P, P, P, P, I64, I64, P, I64, I64, P, I64, I64, I64, P])
    assert sig["moda_fold_rows"] == (C.c_int, [I32, PP, P, P, P, PP, P, P, P, PP, PP, P, PP, P])
    assert sig["moda_mc_emit"] == (C.c_int, [P, P, I64, I64, I64, F32, P, P, P, P] + [F64] * 6 + [I64, I64, P, P, P])
    assert sig["moda_adamw_step"] == (C.c_int, [P] * 5 + [I32, P, P, I32, P, I32, I64] + [F64] * 7 + [P] * 4 + [I64, P, P, P, I32, P])
    assert sig["moda_clip_grad"][1][0] is P           # float* const* in the header, but a table in device memory (as adamw's two)
    assert sig["moda_stream_capture_id"][0] is C.c_uint64 and sig["moda_nn_splits"][0] is I32
    assert sig["moda_loss_assembly"][1][0] is C.POINTER(_lib.AsmTerm) and sig["moda_gemm_f32_ex"][1][0] is C.POINTER(_lib.GemmDesc)
    lib = _lib.load()
    assert lib.moda_mc_emit.argtypes == sig["moda_mc_emit"][1] and lib.moda_nn_splits.restype is I32


def test_struct_layouts_are_the_compilers(tmp_path):
    """sizeof and every offsetof, printed by a host-only C++ program that includes the header, against the ctypes structs."""
    lines = [f'    std::printf("{c} {f} %zu\\n", offsetof({c}, {f}));' for c in abi.STRUCTS for _, f, _ in abi.STRUCTS[c]]
    lines += [f'    std::printf("{c} sizeof %zu\\n", sizeof({c}));' for c in abi.STRUCTS]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "moda_hip.h"\nint main() {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    got = {(c, f): int(v) for c, f, v in (line.split() for line in out.splitlines())}
    want = {(c, "sizeof"): C.sizeof(s) for c, s in STRUCTS.items()}
    want.update({(c, f): getattr(s, f).offset for c, s in STRUCTS.items() for f, _ in s._fields_})
    assert got == want and len(want) == 8 + 27 + 14 + 10 + 4
    assert [f for f, _ in _lib.GemmDesc._fields_][20:24] == ["act", "accumulate", "split_k", "reserved"]
    assert _lib.MlpDesc.window.size == 64 and _lib.NerfTrainDesc.window.size == 64


GOOD = "typedef struct { int32_t a, b; float w[4]; const float* p; } moda_d;\nint moda_f(const moda_d* d, int64_t n, void* stream);\n"


@pytest.mark.parametrize("bad, match", [
    (GOOD.replace("int64_t n", "size_t n"), "size_t"),                          # a parameter of an unknown type
    (GOOD.replace("stream);", "stream)") + "int moda_g(void);\n", "moda_f"),     # an unterminated prototype, another one behind it
    (GOOD.replace("stream);", "stream"), "moda_f"),                             # ... and at the end of the text
    (GOOD.replace("float w[4]", "half w[4]"), "half"),                          # a struct field of an unknown type
    (GOOD + "#define MODA_X (1 << 3)\n", "MODA_X"),                              # a macro whose value is not an integer literal
])
def test_parser_refuses_what_it_does_not_understand(bad, match):
    protos, structs, _ = abi.parse(GOOD)
    assert protos == {"moda_f": ("int", [("const moda_d*", "d"), ("int64_t", "n"), ("void*", "stream")])}
    assert structs == {"moda_d": [("int32_t", "a", None), ("int32_t", "b", None), ("float", "w", 4), ("const float*", "p", None)]}
    with pytest.raises(ValueError, match=match):
        abi.parse(bad)


def test_signatures_follow_the_header(header):
    m = re.search(r"int moda_points_fwd\([^;]*;", header)
    edited = header.replace(m[0], m[0].replace("int64_t S", "int32_t S"))
    assert edited != header
    old, new = _lib._SIGNATURES, _lib.signatures(abi.parse(edited)[0])
    assert [k for k in old if old[k] != new[k]] == ["moda_points_fwd"]
    (res0, args0), (res1, args1) = old["moda_points_fwd"], new["moda_points_fwd"]
    assert res0 is res1 and [i for i, (a, b) in enumerate(zip(args0, args1)) if a is not b] == [4]
    assert args0[4] is I64 and args1[4] is I32 and len(args0) == len(args1) == 7


def test_abi_imports_without_torch_or_ctypes():
    """`import moda_amd.abi` in a fresh interpreter.  The package's own __init__ imports torch (it re-exports the whole call
    surface), so the package is entered as a bare namespace here: what is checked is what abi.py and mlp_pack.py pull in."""
    code = ("import sys, types\n"
            "pkg = types.ModuleType('moda_amd'); pkg.__path__ = [sys.argv[1]]; sys.modules['moda_amd'] = pkg\n"
            "import moda_amd.abi\n"
            "assert 'torch' not in sys.modules and 'ctypes' not in sys.modules, sorted(sys.modules)\n"
            "import moda_amd.mlp_pack\n"
            "assert 'torch' not in sys.modules\n"
            "print(len(moda_amd.abi.PROTOTYPES), moda_amd.mlp_pack.MLP_F16)\n")
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "moda_amd")], capture_output=True, text=True, cwd=ROOT,
                       timeout=300)
    assert (p.returncode, p.stdout.strip()) == (0, "141 32"), p.stderr
