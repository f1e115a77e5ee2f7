"""ctypes binding of libmoda_hip.so (include/moda_hip.h).  The HIP library is the ONLY compute path of
this package: if it is missing, or a tensor is not on a GPU, calls fail loudly -- there is no CPU fallback."""
import ctypes
import os

import torch

from . import abi
from .build import LIB_PATH

_c = ctypes
_I64, _I32, _F32, _P = _c.c_int64, _c.c_int32, _c.c_float, _c.c_void_p

_SCALAR = {"int": _c.c_int, "int32_t": _I32, "int64_t": _I64, "uint32_t": _c.c_uint32, "uint64_t": _c.c_uint64, "float": _F32,
           "double": _c.c_double}
_STRUCT = {}
# `T* const*` parameters that are pointer tables in DEVICE memory, passed by address like any tensor: plain c_void_p.  (As a
# POINTER(c_void_p) argument ctypes would take the c_void_p of `ptr()` for the table itself and pass the address of that object.)
_DEVICE_TABLES = {("moda_clip_grad", "seg_ptr"), ("moda_adamw_step", "seg_p"), ("moda_adamw_step", "seg_g")}


def _ctype(t):
    """The ctypes type of a header type (abi's spelling).  The header cannot tell a host array from a device pointer, so every
    pointer is a c_void_p (it takes tensors' addresses, ctypes arrays and byref alike) but two kinds: a descriptor struct's,
    and a host array of pointers (`T* const*`)."""
    if t.endswith("*const*"):
        return _c.POINTER(_P)
    if t.endswith("*"):
        base = t[:-1].replace("const ", "")
        return _c.POINTER(_STRUCT[base]) if base in _STRUCT else _P
    return _SCALAR[t]


def _struct(name, c_name):
    fields = [(f, _ctype(t) * n if n else _ctype(t)) for t, f, n in abi.STRUCTS[c_name]]
    _STRUCT[c_name] = type(name, (_c.Structure,), {"_fields_": fields})
    return _STRUCT[c_name]


MlpDesc = _struct("MlpDesc", "moda_mlp_desc")
GemmDesc = _struct("GemmDesc", "moda_gemm_desc")
NerfTrainDesc = _struct("NerfTrainDesc", "moda_nerf_train_desc")
AsmTerm = _struct("AsmTerm", "moda_asm_term")


def signatures(prototypes):
    """name -> (restype, argtypes) of parsed prototypes: a new entry point is declared in moda_hip.h and nowhere else."""
    return {name: (_ctype(res), [_P if (name, p) in _DEVICE_TABLES else _ctype(t) for t, p in params])
            for name, (res, params) in prototypes.items()}


_SIGNATURES = signatures(abi.PROTOTYPES)
EXPORTS = tuple(_SIGNATURES)
_VIS_SIGNATURES = signatures(abi.VIS_PROTOTYPES)          # include/moda_hip_vis.h: the same library, a table of its own
VIS_EXPORTS = tuple(_VIS_SIGNATURES)
_CAM_SIGNATURES = signatures(abi.CAM_PROTOTYPES)          # include/moda_hip_cams.h: likewise
CAM_EXPORTS = tuple(_CAM_SIGNATURES)
_SEQVIS_SIGNATURES = signatures(abi.SEQVIS_PROTOTYPES)    # include/moda_hip_seqvis.h: likewise
SEQVIS_EXPORTS = tuple(_SEQVIS_SIGNATURES)
ABI_VERSION = 11       # moda_abi_version() of the library this package was written against (include/moda_hip.h)
_lib = None


def load():
    """Load the shared library (no GPU needed for loading)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m moda_amd.build` (hipcc, gfx950). "
                "moda_amd has no CPU or PyTorch fallback.")
        lib = _c.CDLL(LIB_PATH)
        for name, (res, args) in (list(_SIGNATURES.items()) + list(_VIS_SIGNATURES.items()) + list(_CAM_SIGNATURES.items())
                                  + list(_SEQVIS_SIGNATURES.items())):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.moda_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has ABI version {lib.moda_abi_version()}, this package binds version "
                               f"{ABI_VERSION}: rebuild it with `python -m moda_amd.build`")
        _check_agpr_audit()
        _lib = lib
    return _lib


def _check_agpr_audit():
    """The default 8 x 256 inference kernels own their AGPRs and wait states in inline asm (mlp_fused.hip); the build audits their
    machine code and stamps the verdict (build.audit_built_library).  No stamp, a stamp of other sources, or a failed audit: the
    dispatch takes the compiler-scheduled eight-wave form instead (the library reads MODA_MLP_AGPR per call)."""
    import warnings
    from . import build
    if os.environ.get("MODA_LIB_PATH") or "MODA_MLP_AGPR" in os.environ:
        return                                   # an A/B build or an explicit choice: the caller's business
    try:
        lines = open(build.AUDIT_STAMP).read().splitlines()
    except OSError:
        lines = ["missing"]
    if lines[0] == "ok" and lines[-1] == build.source_hash():
        return
    os.environ["MODA_MLP_AGPR"] = "0"
    warnings.warn("moda_amd: the ISA audit of the AGPR-form 8x256 kernels is " + (lines[0] if lines[0] != "ok" else "of other sources")
                  + " -- using the compiler-scheduled eight-wave kernels (slower, always safe); rebuild with `python -m moda_amd.build`")


def call(name, *args):
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed with code {rc}")


def stream():
    return _c.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(t, dtype=torch.float32):
    """A contiguous device tensor of `dtype`, or an error: the kernels only read GPU memory."""
    if not torch.is_tensor(t):
        raise TypeError(f"expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError("moda_amd ops take CUDA (ROCm) tensors; the HIP library is the only compute path")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def ptr(t):
    return None if t is None else _c.c_void_p(t.data_ptr())


def no_grad_only(*tensors):
    """For entry points that have no backward kernel (the fused inference kernels, the algebra helpers):
    refuse loudly rather than return tensors without a graph.  The differentiable route is moda_amd/autograd.py."""
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError(
            "this moda_amd entry point is inference-only: call it under torch.no_grad(), or use render_rays / "
            "NeRF.forward / Embedding.forward, which switch to the autograd route")


# ---- optional per-launch timing with events on the launch stream (bench.py's roofline leg) ----------
PROFILE = None   # None, or dict: kernel tag -> list of (start_event, end_event, units)


def profile_begin():
    if PROFILE is None:
        return None
    ev = torch.cuda.Event(enable_timing=True)
    ev.record(torch.cuda.current_stream())
    return ev


def profile_end(start, tag, units):
    if start is None:
        return
    end = torch.cuda.Event(enable_timing=True)
    end.record(torch.cuda.current_stream())
    PROFILE.setdefault(tag, []).append((start, end, units))


# ---- small constant tensors (bounds, lattices): built once per (device, values) so that steady-state calls issue no
#      host-to-device copy (which would also be illegal while a HIP graph is being captured) ----------------------------
_CONST = {}


def const_tensor(key, device, make):
    """Cached device tensor for an immutable host-side constant; `make()` returns a CPU tensor / array."""
    k = (key, str(device))
    t = _CONST.get(k)
    if t is None:
        v = make()
        t = (v if torch.is_tensor(v) else torch.as_tensor(v)).to(device=device, dtype=torch.float32).contiguous()
        _CONST[k] = t
    return t
