"""The internal entry points of the bf16-storage backward (moda_amd/csrc/moda_dev.h: moda_bwd256_layer, moda_chain64_bwd,
moda_chain64_part_floats, moda_heads64_bwd, moda_pe_ends64_bwd) for the tests that drive them with crafted operands.  They have C++
linkage and are exported from libmoda_hip.so (the build sets no visibility flag) but are no part of the C ABI, so their mangled
names are looked up in the library's ELF dynamic symbol table (.dynsym / .dynstr, read here: no `nm` needed where the tests run) by
the length-prefixed identifier of the Itanium mangling (`_Z17moda_bwd256_layer...`), exactly one match each, and restype / argtypes
are set from the declarations in moda_dev.h:
  T* const*            a HOST array of device pointers            POINTER(c_void_p)
  const long long*     a HOST array                               POINTER(c_longlong)
  any other pointer    c_void_p (device memory; `window` of moda_pe_ends64_bwd is a host float array, a ctypes array passes as one)
  int / long long      c_int / c_longlong"""
import ctypes
import os
import re
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_HEADER = os.path.join(ROOT, "moda_amd", "csrc", "moda_dev.h")
ENTRIES = ("moda_bwd256_layer", "moda_chain64_bwd", "moda_chain64_part_floats", "moda_heads64_bwd", "moda_pe_ends64_bwd")

SHT_DYNSYM = 11


def dynamic_symbols(path):
    """Names of the DEFINED symbols of an ELF64 little-endian file's dynamic symbol table."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
        raise ValueError(f"{path}: not a little-endian ELF64 file")
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = []
    for (_, sh_type, _, _, off, size, link, _, _, entsize) in sections:
        if sh_type != SHT_DYNSYM:
            continue
        str_off, str_size = sections[link][4], sections[link][5]
        strtab = data[str_off:str_off + str_size]
        for o in range(off, off + size, entsize or 24):
            st_name, _, _, st_shndx, _, _ = struct.unpack_from("<IBBHQQ", data, o)
            if st_shndx == 0 or st_name == 0:
                continue
            names.append(strtab[st_name:strtab.index(b"\0", st_name)].decode())
    return names


def mangled(names, ident):
    """The one symbol of `names` that is the function `ident` at namespace scope."""
    hits = [n for n in names if n.startswith(f"_Z{len(ident)}{ident}")]
    assert len(hits) == 1, (ident, hits)
    return hits[0]


TYPE_WORDS = frozenset(("const", "void", "int", "long", "float"))


def parameter_type(p):
    """The type of one parameter declaration: its name, when it has one, dropped.  Every word left must be a type word."""
    words = re.findall(r"\w+|\*", p)
    if words and words[-1] != "*" and words[-1] not in TYPE_WORDS:
        words.pop()
    assert words and all(w == "*" or w in TYPE_WORDS for w in words), p
    return " ".join(words).replace(" *", "*")


def declarations(header=DEV_HEADER):
    """ident -> (return type, [parameter type, ...]) of the five entries, as moda_dev.h declares them."""
    with open(header) as f:
        text = re.sub(r"/\*.*?\*/", " ", re.sub(r"//[^\n]*", "", f.read()), flags=re.S)
    out = {}
    for ident in ENTRIES:
        m = re.findall(r"\b(int|long long)\s+" + ident + r"\s*\(([^)]*)\)\s*;", text)
        assert len(m) == 1, (ident, m)
        out[ident] = (m[0][0], [parameter_type(p) for p in m[0][1].split(",")])
    return out


def ctype(t):
    t = t.replace(" ", "")
    if t.endswith("*const*"):
        return ctypes.POINTER(ctypes.c_void_p)
    if t == "constlonglong*":
        return ctypes.POINTER(ctypes.c_longlong)
    if t.endswith("*"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "longlong": ctypes.c_longlong}[t]


def signatures():
    return {k: (ctype(res), [ctype(p) for p in params]) for k, (res, params) in declarations().items()}


def bind(lib, path):
    """ident -> the ctypes function of `lib` (the CDLL of `path`) with restype and argtypes set."""
    names = dynamic_symbols(path)
    fns = {}
    for ident, (res, args) in signatures().items():
        fn = getattr(lib, mangled(names, ident))
        fn.restype, fn.argtypes = res, args
        fns[ident] = fn
    return fns


_FNS = None


def entries():
    """The five entries of the package's own library."""
    global _FNS
    if _FNS is None:
        from moda_amd import _lib
        _FNS = bind(_lib.load(), _lib.LIB_PATH)
    return _FNS
