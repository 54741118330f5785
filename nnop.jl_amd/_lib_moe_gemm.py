"""ctypes binding of libnnop_hip_moe_gemm.so (the C ABI of include/nnop_hip_moe_gemm.h): the grouped GEMM over the MoE dispatch plan.

The fifth library has an ABI version of its own; dtypes, status codes and their messages are the main library's (``_lib``).
There is NO fallback: if the shared library is missing, has another moe-gemm-ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import NNopLibraryMissing

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_moe_gemm.so")

# NNOP_HIP_MOE_GEMM_ABI_VERSION of the header this binding was written against; load() refuses another library
MOE_GEMM_ABI_VERSION = 1

EXPORTED_SYMBOLS = (
    "nnop_moe_gemm_abi_version",
    "nnop_moe_gemm",
    "nnop_moe_gemm_bwd_x",
    "nnop_moe_gemm_bwd_w",
)

MAX_EXPERTS, MAX_DIM = 1024, 65536


class MoeGemmDesc(C.Structure):
    """struct nnop_moe_gemm_desc"""
    _fields_ = [("dtype", C.c_int32), ("rows", C.c_int32), ("experts", C.c_int32), ("in_dim", C.c_int32), ("out_dim", C.c_int32),
                ("ld_x", C.c_int32), ("ld_y", C.c_int32), ("ld_w", C.c_int32), ("reserved", C.c_int32 * 2)]


_lib = None


def load():
    """dlopen the library once and declare the prototypes.  Raises loudly when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NNopLibraryMissing(
            f"{LIB_PATH} not found: build it with `make -C nnop.jl_amd/csrc -j8` "
            "(or __graft_entry__.build()).  There is no CPU or PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    if not hasattr(lib, "nnop_moe_gemm_abi_version"):
        raise NNopLibraryMissing(f"{LIB_PATH} exports no nnop_moe_gemm_abi_version: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    lib.nnop_moe_gemm_abi_version.restype = C.c_int
    lib.nnop_moe_gemm_abi_version.argtypes = []
    if lib.nnop_moe_gemm_abi_version() != MOE_GEMM_ABI_VERSION:
        raise NNopLibraryMissing(f"{LIB_PATH} has moe-gemm-ABI version {lib.nnop_moe_gemm_abi_version()}, this binding needs "
                                 f"{MOE_GEMM_ABI_VERSION}: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    for name in EXPORTED_SYMBOLS:
        if not hasattr(lib, name):
            raise NNopLibraryMissing(f"{LIB_PATH} does not export {name}: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    vp, gd = C.c_void_p, C.POINTER(MoeGemmDesc)
    for name in EXPORTED_SYMBOLS[1:]:
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [gd, vp, vp, vp, vp, vp]
    _lib = lib
    return lib
