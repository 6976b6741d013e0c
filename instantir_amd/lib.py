"""ctypes binding of libinstantir_hip.so, derived from include/instantir_hip.h (the C ABI) when this module is imported.

The header is the single source: `cheader.parse_file` reads it once per process and everything here is taken from the result
-- the descriptor classes (generated `ctypes.Structure`s under their Python names), `SIGNATURES`, and `MACROS`, the integer
`IIR_*` macros that the constants of this and the other host modules are looked up in.  Nothing is copied by hand, so a field,
an argument or a limit changes in the header alone.  Importing this module needs neither torch nor a GPU.

The library is the product: there is no PyTorch / CPU fallback.  `load()` raises if the shared object is missing or does not
export a declared symbol, and the callers pass every return code through `check()`.
"""
from __future__ import annotations

import ctypes as C
import os

from .cheader import HipLibraryError, parse_file

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libinstantir_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "instantir_hip.h")

HEADER = parse_file(HEADER_PATH)
MACROS = HEADER.macros

AttnKV, GemmDesc, ConvDesc, AttnDesc, AdaLNJob, SchedDesc, ResampleDesc, MetricsDesc = (HEADER.structs[name] for name in (
    "iir_attn_kv", "iir_gemm_desc", "iir_conv_desc", "iir_attn_desc", "iir_adaln_job", "iir_sched_desc", "IirResampleDesc",
    "iir_metrics_desc"))

EPI_PLAIN, EPI_GEGLU, EPI_SFT, EPI_XATTN = (MACROS["IIR_EPI_" + n] for n in ("PLAIN", "GEGLU", "SFT", "XATTN"))
ACT_NONE, ACT_SILU, ACT_GELU, ACT_QUICKGELU = (MACROS["IIR_ACT_" + n] for n in ("NONE", "SILU", "GELU", "QUICKGELU"))
STEP_PAG, STEP_HIST, STEP_KEEP, STEP_APG = (MACROS["IIR_STEP_" + n] for n in ("PAG", "HIST", "KEEP", "APG"))   # SchedDesc.groups
METRIC_PSNR, METRIC_SSIM = MACROS["IIR_METRIC_PSNR"], MACROS["IIR_METRIC_SSIM"]                                # MetricsDesc.what

# The one exception to cheader's type rule, as (function, parameter): a struct table that lives in DEVICE memory.  The caller
# has its address as an integer (tensor.data_ptr()), which POINTER(struct) refuses, so it is bound as a raw address.
DEVICE_TABLES = {("iir_adaln_batch_f16", "jobs_dev")}

# symbol -> (restype, argtypes) of every function the header declares
SIGNATURES = {fn: (restype, [C.c_void_p if (fn, p) in DEVICE_TABLES else ct for p, ct in params])
              for fn, (restype, params) in HEADER.functions.items()}

_lib = None


def declared_symbols(header_path: str = HEADER_PATH):
    """Function names declared in include/instantir_hip.h."""
    return sorted(HEADER.functions if header_path == HEADER_PATH else parse_file(header_path).functions)


def load():
    """dlopen the in-tree library and bind every declared symbol; raises HipLibraryError otherwise."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64.so.7; importing it first makes our library bind to that same
    # runtime instance (one HIP runtime per process), otherwise torch streams/pointers are foreign to us.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: build it with instantir_amd/csrc/build.sh (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback for the denoising path.")
    lib = C.CDLL(LIB_PATH)
    for name, signature in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype, fn.argtypes = signature
    if lib.iir_abi_version() != MACROS["IIR_ABI_VERSION"]:
        raise HipLibraryError("ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        raise HipLibraryError(f"{what} failed with code {rc} ({'invalid argument' if rc == -1 else 'launch failure'})")
