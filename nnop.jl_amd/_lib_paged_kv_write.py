"""ctypes binding of libnnop_hip_paged_kv_write.so (the C ABI of include/nnop_hip_paged_kv_write.h): the write side of the paged KV cache --
the new tokens' K and V rows into the pages that the paged attention calls read, as they are or as E4M3 codes.

The seventeenth library has an ABI version of its own; dtypes, status codes and their messages are the main library's (``_lib``), and so
is the load sequence (``_lib.load_library``).
There is NO fallback: if the shared library is missing, has another paged-kv-write-ABI version or lacks a symbol, load() raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnnop_hip_paged_kv_write.so")

# NNOP_HIP_PAGED_KV_WRITE_ABI_VERSION of the header this binding was written against; load() refuses another library
PAGED_KV_WRITE_ABI_VERSION = 1

BLOCK_TOKENS, MIN_PAGE_SIZE = 4, 16                   # NNOP_PAGED_KV_WRITE_BLOCK_TOKENS, _MIN_PAGE_SIZE
KV_16BIT, KV_E4M3 = 0, 1                               # NNOP_PAGED_KV_WRITE_16BIT, _E4M3
EMBS = (64, 128)


class PagedKvWriteDesc(C.Structure):
    """struct nnop_paged_kv_write_desc"""
    _fields_ = [("dtype", C.c_int32), ("emb", C.c_int32), ("tokens", C.c_int32), ("kh", C.c_int32), ("batch", C.c_int32),
                ("max_pages", C.c_int32), ("page_size", C.c_int32), ("num_pages", C.c_int32), ("kv_format", C.c_int32),
                ("reserved", C.c_int32), ("flags", C.c_uint32), ("reserved2", C.c_int32),
                ("kp_stride_p", C.c_int64), ("kp_stride_h", C.c_int64), ("kp_stride_l", C.c_int64),
                ("vp_stride_p", C.c_int64), ("vp_stride_h", C.c_int64), ("vp_stride_l", C.c_int64), ("table_stride", C.c_int64),
                ("k_stride_t", C.c_int64), ("k_stride_h", C.c_int64), ("v_stride_t", C.c_int64), ("v_stride_h", C.c_int64)]


_vp, _ld = C.c_void_p, C.POINTER(PagedKvWriteDesc)

# name -> (restype, argtypes) of every function of the header; EXPORTED_SYMBOLS is its keys
PROTOTYPES = {
    "nnop_paged_kv_write_abi_version": (C.c_int, []),
    "nnop_paged_kv_write": (C.c_int, [_ld, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

_lib = None


def load():
    """dlopen the library once and declare the prototypes.  Raises loudly when absent."""
    if _lib is not None:
        return _lib
    return load_library(sys.modules[__name__], "paged-kv-write-ABI version", "PAGED_KV_WRITE_ABI_VERSION", "nnop_paged_kv_write_abi_version")
