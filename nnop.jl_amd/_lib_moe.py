"""ctypes binding of libnnop_hip_moe.so (the C ABI of include/nnop_hip_moe.h): mixture-of-experts routing.

The third library has an ABI version of its own; dtypes, status codes and their messages are the main library's (``_lib``).
There is NO fallback: if the shared library is missing, has another moe-ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import NNopLibraryMissing

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_moe.so")

# NNOP_HIP_MOE_ABI_VERSION of the header this binding was written against; load() refuses another library
MOE_ABI_VERSION = 1

EXPORTED_SYMBOLS = (
    "nnop_moe_abi_version",
    "nnop_moe_router",
    "nnop_moe_router_bwd",
    "nnop_moe_plan_workspace_bytes",
    "nnop_moe_plan",
)

# enum nnop_moe_norm
NNOP_MOE_NORM_TOPK, NNOP_MOE_NORM_ALL = 0, 1
NORMS = {"topk": NNOP_MOE_NORM_TOPK, "all": NNOP_MOE_NORM_ALL}
MAX_EXPERTS, MAX_TOPK = 1024, 16


class MoeRouterDesc(C.Structure):
    """struct nnop_moe_router_desc"""
    _fields_ = [("dtype", C.c_int32), ("tokens", C.c_int32), ("experts", C.c_int32), ("topk", C.c_int32), ("ld", C.c_int32),
                ("norm", C.c_int32), ("reserved", C.c_int32 * 2)]


class MoePlanDesc(C.Structure):
    """struct nnop_moe_plan_desc"""
    _fields_ = [("tokens", C.c_int32), ("topk", C.c_int32), ("experts", C.c_int32), ("reserved", C.c_int32 * 1)]


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
    if not hasattr(lib, "nnop_moe_abi_version"):
        raise NNopLibraryMissing(f"{LIB_PATH} exports no nnop_moe_abi_version: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    lib.nnop_moe_abi_version.restype = C.c_int
    lib.nnop_moe_abi_version.argtypes = []
    if lib.nnop_moe_abi_version() != MOE_ABI_VERSION:
        raise NNopLibraryMissing(f"{LIB_PATH} has moe-ABI version {lib.nnop_moe_abi_version()}, this binding needs "
                                 f"{MOE_ABI_VERSION}: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    for name in EXPORTED_SYMBOLS:
        if not hasattr(lib, name):
            raise NNopLibraryMissing(f"{LIB_PATH} does not export {name}: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    vp, rd, pd = C.c_void_p, C.POINTER(MoeRouterDesc), C.POINTER(MoePlanDesc)
    lib.nnop_moe_router.restype = C.c_int
    lib.nnop_moe_router.argtypes = [rd, vp, vp, vp, vp, vp]
    lib.nnop_moe_router_bwd.restype = C.c_int
    lib.nnop_moe_router_bwd.argtypes = [rd, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.nnop_moe_plan_workspace_bytes.restype = C.c_size_t
    lib.nnop_moe_plan_workspace_bytes.argtypes = [pd]
    lib.nnop_moe_plan.restype = C.c_int
    lib.nnop_moe_plan.argtypes = [pd, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    _lib = lib
    return lib
