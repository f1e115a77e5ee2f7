"""include/moda_hip.h, parsed once at import: the header is the only description of the library's C ABI, and _lib.py (ctypes
signatures, descriptor structs) and every module that needs a MODA_* macro's value read it from here.  No torch, no ctypes.

Not a C parser: it knows the header's own regular shape -- `#define MODA_X <integer>`, `typedef struct ... { fields } name;`,
`<scalar> moda_name(<type> <name>, ...);` -- and raises ValueError, with the text it stopped at, on anything else."""
import re

from .build import HEADERS

SCALARS = ("int", "int32_t", "int64_t", "uint32_t", "uint64_t", "float", "double")
_POINTEES = SCALARS + ("void", "uint8_t")


def _type(text, structs, where):
    """'const  float * const *' -> 'const float*const*': a scalar by value, or one or two levels of pointer (the outer one to
    const pointers) to a scalar, a byte, void or one of `structs`."""
    t = re.sub(r"\s*\*\s*", "*", " ".join(text.split()))
    m = re.fullmatch(r"(?:const )?(\w+)(\*(?:const\*)?)?", t)
    if not m or m[1] not in (_POINTEES if m[2] else SCALARS) + tuple(structs):
        raise ValueError(f"moda_hip.h: {where}: unknown type {text!r}")
    return t


def parse(text):
    """(PROTOTYPES, STRUCTS, CONSTANTS) of a header's text."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {}
    for line in re.findall(r"^[ \t]*#.*$", text, flags=re.M):
        m = re.fullmatch(r"\s*#\s*define\s+(\w+)(?:\s+(\S.*?))?\s*", line)
        if m and m[2] is not None:
            v = re.fullmatch(r"\(?(-?(?:0[xX][0-9a-fA-F]+|\d+))\)?", m[2])
            if not v or not m[1].startswith("MODA_"):
                raise ValueError(f"moda_hip.h: not an integer MODA_* macro: {line.strip()!r}")
            constants[m[1]] = int(v[1], 0)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).replace('extern "C" {', "")

    structs = {}

    def struct(m):
        fields = structs[m[2]] = []
        for decl in filter(None, (d.strip() for d in m[1].split(";"))):
            d = re.fullmatch(r"((?:const\s+)?\w+\s*\*?)\s*(\w+(?:\s*\[\d+\])?(?:\s*,\s*\w+(?:\s*\[\d+\])?)*)", decl)
            if not d or ("*" in d[1] and "," in d[2]):
                raise ValueError(f"moda_hip.h: struct {m[2]}: cannot read the field {decl!r}")
            for name, length in re.findall(r"(\w+)(?:\s*\[(\d+)\])?", d[2]):
                fields.append((_type(d[1], (), "struct " + m[2]), name, int(length) if length else None))
        return ""
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)

    *decls, tail = text.split(";")
    if tail.strip() not in ("", "}"):
        raise ValueError(f"moda_hip.h: unterminated declaration {tail.strip()!r}")
    prototypes = {}
    for decl in decls:
        m = re.fullmatch(r"\s*(\w+)\s+(moda_\w+)\s*\((.*)\)\s*", decl, flags=re.S)
        if not m:
            raise ValueError(f"moda_hip.h: not a prototype: {decl.strip()!r}")
        params = []
        if m[3].strip() != "void":
            for p in m[3].split(","):
                q = re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", p, flags=re.S)
                if not q:
                    raise ValueError(f"moda_hip.h: {m[2]}: cannot read the parameter {p.strip()!r}")
                params.append((_type(q[1], structs, m[2]), q[2]))
        prototypes[m[2]] = (_type(m[1], (), m[2]), params)
    return prototypes, structs, constants


with open(next(h for h in HEADERS if h.endswith("moda_hip.h"))) as _f:
    PROTOTYPES, STRUCTS, CONSTANTS = parse(_f.read())
# include/moda_hip_vis.h, the evaluation-frame entries: the same shape, tables of its own (the three above are moda_hip.h's alone)
with open(next(h for h in HEADERS if h.endswith("moda_hip_vis.h"))) as _f:
    VIS_PROTOTYPES, VIS_STRUCTS, VIS_CONSTANTS = parse(_f.read())
# include/moda_hip_cams.h, the camera entries (moda_amd/cams.py): a third header of the same shape, tables of its own
with open(next(h for h in HEADERS if h.endswith("moda_hip_cams.h"))) as _f:
    CAM_PROTOTYPES, CAM_STRUCTS, CAM_CONSTANTS = parse(_f.read())
# include/moda_hip_seqvis.h, the mesh-sequence rendering entries (moda_amd/seq_render.py): a fourth header of the same shape
with open(next(h for h in HEADERS if h.endswith("moda_hip_seqvis.h"))) as _f:
    SEQVIS_PROTOTYPES, SEQVIS_STRUCTS, SEQVIS_CONSTANTS = parse(_f.read())
