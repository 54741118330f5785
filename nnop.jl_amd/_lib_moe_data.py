"""ctypes binding of libnnop_hip_moe_data.so (the C ABI of include/nnop_hip_moe_data.h): the MoE token permute and weighted combine.

The fourth library has an ABI version of its own; dtypes, status codes and their messages are the main library's (``_lib``).
There is NO fallback: if the shared library is missing, has another moe-data-ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import NNopLibraryMissing

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_moe_data.so")

# NNOP_HIP_MOE_DATA_ABI_VERSION of the header this binding was written against; load() refuses another library
MOE_DATA_ABI_VERSION = 1

EXPORTED_SYMBOLS = (
    "nnop_moe_data_abi_version",
    "nnop_moe_permute",
    "nnop_moe_permute_bwd",
    "nnop_moe_combine",
    "nnop_moe_combine_bwd",
)

MAX_TOPK, MAX_DIM = 64, 65536


class MoeRowsDesc(C.Structure):
    """struct nnop_moe_rows_desc"""
    _fields_ = [("dtype", C.c_int32), ("tokens", C.c_int32), ("topk", C.c_int32), ("dim", C.c_int32), ("ld_tok", C.c_int32),
                ("ld_slot", C.c_int32), ("reserved", C.c_int32 * 2)]


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
    if not hasattr(lib, "nnop_moe_data_abi_version"):
        raise NNopLibraryMissing(f"{LIB_PATH} exports no nnop_moe_data_abi_version: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    lib.nnop_moe_data_abi_version.restype = C.c_int
    lib.nnop_moe_data_abi_version.argtypes = []
    if lib.nnop_moe_data_abi_version() != MOE_DATA_ABI_VERSION:
        raise NNopLibraryMissing(f"{LIB_PATH} has moe-data-ABI version {lib.nnop_moe_data_abi_version()}, this binding needs "
                                 f"{MOE_DATA_ABI_VERSION}: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    for name in EXPORTED_SYMBOLS:
        if not hasattr(lib, name):
            raise NNopLibraryMissing(f"{LIB_PATH} does not export {name}: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    vp, rd = C.c_void_p, C.POINTER(MoeRowsDesc)
    lib.nnop_moe_permute.restype = C.c_int
    lib.nnop_moe_permute.argtypes = [rd, vp, vp, vp, vp]
    lib.nnop_moe_permute_bwd.restype = C.c_int
    lib.nnop_moe_permute_bwd.argtypes = [rd, vp, vp, vp, vp]
    lib.nnop_moe_combine.restype = C.c_int
    lib.nnop_moe_combine.argtypes = [rd, vp, vp, vp, vp, vp]
    lib.nnop_moe_combine_bwd.restype = C.c_int
    lib.nnop_moe_combine_bwd.argtypes = [rd, vp, vp, vp, vp, vp, vp, vp, vp]
    _lib = lib
    return lib
