"""ctypes binding of libnnop_hip_ext.so (the C ABI of include/nnop_hip_ext.h): operators beyond the NNop drop-in boundary.

The second library has an ABI version of its own; dtypes, status codes and their messages are the main library's (``_lib``).
There is NO fallback: if the shared library is missing, has another ext-ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import NNopLibraryMissing

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_ext.so")

# NNOP_HIP_EXT_ABI_VERSION of the header this binding was written against; load() refuses another library
EXT_ABI_VERSION = 1

EXPORTED_SYMBOLS = (
    "nnop_ext_abi_version",
    "nnop_qk_norm_rope",
    "nnop_qk_norm_rope_bwd_workspace_bytes",
    "nnop_qk_norm_rope_bwd",
)


class QknrDesc(C.Structure):
    """struct nnop_qknr_desc"""
    _fields_ = [("dtype", C.c_int32), ("w_dtype", C.c_int32), ("cs_dtype", C.c_int32), ("dim", C.c_int32), ("seq", C.c_int32),
                ("qh", C.c_int32), ("kh", C.c_int32), ("batch", C.c_int32), ("eps", C.c_float), ("offset", C.c_float),
                ("reserved", C.c_int32 * 2)]


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
    if not hasattr(lib, "nnop_ext_abi_version"):
        raise NNopLibraryMissing(f"{LIB_PATH} exports no nnop_ext_abi_version: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    lib.nnop_ext_abi_version.restype = C.c_int
    lib.nnop_ext_abi_version.argtypes = []
    if lib.nnop_ext_abi_version() != EXT_ABI_VERSION:
        raise NNopLibraryMissing(f"{LIB_PATH} has ext-ABI version {lib.nnop_ext_abi_version()}, this binding needs "
                                 f"{EXT_ABI_VERSION}: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    for name in EXPORTED_SYMBOLS:
        if not hasattr(lib, name):
            raise NNopLibraryMissing(f"{LIB_PATH} does not export {name}: rebuild with `make -C nnop.jl_amd/csrc -j8`")
    vp, qd = C.c_void_p, C.POINTER(QknrDesc)
    lib.nnop_qk_norm_rope.restype = C.c_int
    lib.nnop_qk_norm_rope.argtypes = [qd, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.nnop_qk_norm_rope_bwd_workspace_bytes.restype = C.c_size_t
    lib.nnop_qk_norm_rope_bwd_workspace_bytes.argtypes = [qd]
    lib.nnop_qk_norm_rope_bwd.restype = C.c_int
    lib.nnop_qk_norm_rope_bwd.argtypes = [qd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    _lib = lib
    return lib
