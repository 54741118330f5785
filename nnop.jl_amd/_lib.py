"""ctypes binding of libnnop_hip.so (the C ABI of include/nnop_hip.h).

This is the same binding, call for call, that the Julia extension in ``julia/NNopHIPExt.jl``
makes with ``ccall``.  There is NO fallback: if the shared library is missing or a symbol is
absent the import of the product path raises.  ``load_library`` is the load sequence of this binding and of the four
side bindings (``_lib_ext``, ``_lib_moe``, ``_lib_moe_data``, ``_lib_moe_gemm``).
"""
from __future__ import annotations

import ctypes as C
import numbers
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# NNOP_LIB_PATH: development override (timing-only ablation builds); never set in production
LIB_PATH = os.environ.get("NNOP_LIB_PATH") or os.path.join(_HERE, "lib", "libnnop_hip.so")

# NNOP_HIP_ABI_VERSION of the header this binding was written against; load() refuses another library
ABI_VERSION = 7

# nnop_dtype (include/nnop_hip.h)
NNOP_F32, NNOP_F16, NNOP_BF16 = 0, 1, 2

# nnop_status (include/nnop_hip.h)
NNOP_OK = 0
NNOP_ERR_EMB_MISMATCH = -1
NNOP_ERR_KV_SHAPE = -2
NNOP_ERR_EMB_NOT_POW2 = -3
NNOP_ERR_HEADS = -4
NNOP_ERR_DTYPE = -5
NNOP_ERR_NULL = -6
NNOP_ERR_EMB_UNSUPPORTED = -7
NNOP_ERR_SHAPE = -8
NNOP_ERR_WORKSPACE = -9
NNOP_ERR_HIP = -10
NNOP_ERR_ALIGN = -11
NNOP_ERR_OPTS = -12

# what the test-only hooks (csrc/nnop_debug.h; DEBUG_PROTOTYPES below) report and take
FWD_FORMS = {0: "fa_fwd_kernel", 1: "fa_fwd_split_kernel", 2: "fa_fwd_w64_kernel", 3: "fa_fwd_generic_kernel", 4: "fa_fwd_duo_kernel"}
FWD_FORMS_CAP = {0: "fa_fwd_cap_kernel", 3: "fa_fwd_generic_cap_kernel"}      # a capped call runs these two forms only; form names, not symbols (fwd_form)
# keys of nnop_debug_set == enum TuneKey (csrc/tuning.hpp)
TUNE_KEYS = {"fwd_split": 0, "fwd_nw": 1, "fwd_w64": 2, "bwd_big7": 3, "norm_bwd_cap": 4, "bwd_nw": 5,
             "fwd_exact_scale": 6, "bwd_w64": 7, "bwd_stages": 8, "fwd_persist": 9, "bwd_persist": 10, "fwd_duo": 11, "fwd_persist_asc": 12, "bwd_narrow": 13, "fwd_causal_alt": 14}


class FaShard(C.Structure):
    """struct nnop_fa_shard (declared below FaDesc; fields filled in after it)"""


class FaDesc(C.Structure):
    """struct nnop_fa_desc"""
    _fields_ = [
        ("dtype", C.c_int32), ("emb", C.c_int32), ("ql", C.c_int32), ("kl", C.c_int32),
        ("qh", C.c_int32), ("kh", C.c_int32), ("batch", C.c_int32), ("causal", C.c_int32),
        ("emb_k", C.c_int32), ("emb_v", C.c_int32), ("kl_v", C.c_int32), ("kh_v", C.c_int32),
    ]


FaShard._fields_ = [("desc", FaDesc), ("b0", C.c_int32), ("b1", C.c_int32), ("kh0", C.c_int32), ("kh1", C.c_int32),
                    ("q_off", C.c_uint64), ("kv_off", C.c_uint64), ("row_off", C.c_uint64), ("mask_off", C.c_uint64),
                    ("pair_off", C.c_int64)]


class FaOpts(C.Structure):
    """struct nnop_fa_opts (ABI version 7): per-call options of nnop_fa_fwd_ex / nnop_fa_bwd_ex"""
    _fields_ = [("window_left", C.c_int32), ("window_right", C.c_int32), ("reserved", C.c_int32 * 6)]


class RopeDesc(C.Structure):
    """struct nnop_rope_desc"""
    _fields_ = [
        ("dtype", C.c_int32), ("cs_dtype", C.c_int32), ("dim", C.c_int32), ("seq", C.c_int32),
        ("qh", C.c_int32), ("kh", C.c_int32), ("batch", C.c_int32),
    ]


class SoftmaxDesc(C.Structure):
    """struct nnop_softmax_desc"""
    _fields_ = [("dtype", C.c_int32), ("n", C.c_int32), ("batch", C.c_int64)]


class NormDesc(C.Structure):
    """struct nnop_norm_desc"""
    _fields_ = [("dtype", C.c_int32), ("w_dtype", C.c_int32), ("emb", C.c_int32), ("reserved", C.c_int32),
                ("n", C.c_int64)]


# nnop_glu_act / nnop_glu_layout (include/nnop_hip.h)
GLU_ACTS = {"silu": 0, "gelu_tanh": 1, "gelu_erf": 2, "swiglu_oai": 3}
GLU_SPLIT, GLU_INTERLEAVED = 0, 1


class GluDesc(C.Structure):
    """struct nnop_glu_desc"""
    _fields_ = [("dtype", C.c_int32), ("act", C.c_int32), ("layout", C.c_int32), ("reserved", C.c_int32),
                ("rows", C.c_int64), ("n", C.c_int64), ("ld", C.c_int64), ("alpha", C.c_float), ("limit", C.c_float)]


class XentDesc(C.Structure):
    """struct nnop_xent_desc"""
    _fields_ = [("dtype", C.c_int32), ("index_bytes", C.c_int32), ("rows", C.c_int64), ("n", C.c_int64), ("ld", C.c_int64),
                ("ld_grad", C.c_int64), ("ignore_index", C.c_int64), ("index_base", C.c_int32), ("reserved", C.c_int32),
                ("label_smoothing", C.c_float), ("z_loss", C.c_float), ("softcap", C.c_float), ("reserved_f", C.c_float)]


class NNopLibraryMissing(ImportError):
    pass


_vp = _u8p = C.c_void_p
_fd, _op, _nd, _gd, _xd = C.POINTER(FaDesc), C.POINTER(FaOpts), C.POINTER(NormDesc), C.POINTER(GluDesc), C.POINTER(XentDesc)

# name -> (restype, argtypes) of every function of include/nnop_hip.h.  load() declares them from this table and refuses a library
# that lacks one; EXPORTED_SYMBOLS is its keys, so the symbol list and the prototypes cannot drift apart.
PROTOTYPES = {
    "nnop_fa_fwd": (C.c_int, [_fd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u8p, _vp]),
    "nnop_fa_bwd_workspace_bytes": (C.c_size_t, [_fd]),
    "nnop_fa_bwd_workspace_bytes_pair": (C.c_size_t, [_fd]),
    "nnop_fa_bwd": (C.c_int, [_fd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u8p, _vp, C.c_size_t, _vp]),
    "nnop_fa_fwd_ex": (C.c_int, [_fd, _op, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u8p, _vp]),
    "nnop_fa_bwd_ex": (C.c_int, [_fd, _op, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u8p, _vp, C.c_size_t, _vp]),
    "nnop_fa_fwd_sinks": (C.c_int, [_fd, _op, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u8p, _vp]),
    "nnop_fa_bwd_sinks": (C.c_int, [_fd, _op, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u8p, _vp,
                                    C.c_size_t, _vp]),
    "nnop_fa_fwd_softcap": (C.c_int, [_fd, _op, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u8p, _vp]),
    "nnop_fa_bwd_softcap": (C.c_int, [_fd, _op, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u8p,
                                      _vp, C.c_size_t, _vp]),
    "nnop_llama_rope": (C.c_int, [C.POINTER(RopeDesc), _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp]),
    "nnop_online_softmax": (C.c_int, [C.POINTER(SoftmaxDesc), _vp, _vp, _vp]),
    "nnop_online_softmax_bwd": (C.c_int, [C.POINTER(SoftmaxDesc), _vp, _vp, _vp, _vp]),
    "nnop_rms_norm": (C.c_int, [_nd, _vp, _vp, _vp, _vp, C.c_float, C.c_float, _vp]),
    "nnop_rms_norm_bwd": (C.c_int, [_nd, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp, C.c_size_t, _vp]),
    "nnop_layer_norm": (C.c_int, [_nd, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp]),
    "nnop_layer_norm_bwd": (C.c_int, [_nd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "nnop_norm_bwd_workspace_bytes": (C.c_size_t, [_nd, C.c_int]),
    "nnop_add_rms_norm": (C.c_int, [_nd, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, C.c_float, _vp]),
    "nnop_add_rms_norm_bwd": (C.c_int, [_nd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp, C.c_size_t, _vp]),
    "nnop_add_layer_norm": (C.c_int, [_nd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp]),
    "nnop_add_layer_norm_bwd": (C.c_int, [_nd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "nnop_glu": (C.c_int, [_gd, _vp, _vp, _vp, _vp]),
    "nnop_glu_bwd": (C.c_int, [_gd, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nnop_cross_entropy": (C.c_int, [_xd, _vp, _vp, _vp, _vp, _vp]),
    "nnop_cross_entropy_bwd": (C.c_int, [_xd, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nnop_fa_shards": (C.c_int, [_fd, C.c_int, C.c_int, C.POINTER(FaShard)]),
    "nnop_shared_memory": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "nnop_strerror": (C.c_char_p, [C.c_int]),
    "nnop_abi_version": (C.c_int, []),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

# Test-only hooks (csrc/nnop_debug.h): exported by the library, deliberately NOT in the public header and not part of the ABI;
# each is bound only when the library carries it.
DEBUG_PROTOTYPES = {
    "nnop_debug_set": (C.c_int, [C.c_int, C.c_int]),
    "nnop_debug_dev_build": (C.c_int, []),
    "nnop_debug_fwd_form": (C.c_int, [_fd, C.c_int, C.c_int]),
    "nnop_debug_bwd_form": (C.c_int, [_fd, C.c_int, C.c_int]),
    "nnop_debug_fwd_form_ex": (C.c_int, [_fd, _op, C.c_int, C.c_int]),
    "nnop_debug_bwd_form_ex": (C.c_int, [_fd, _op, C.c_int, C.c_int]),
    "nnop_debug_fwd_form_cap": (C.c_int, [_fd, _op, C.c_float, C.c_int, C.c_int]),
    "nnop_debug_bwd_form_cap": (C.c_int, [_fd, _op, C.c_float, C.c_int, C.c_int]),
}
DEBUG_SYMBOLS = tuple(DEBUG_PROTOTYPES)


def load_library(binding, label, version_name, version_symbol, optional=None):
    """The load sequence of all nine bindings.  `binding` is the binding module: its LIB_PATH, EXPORTED_SYMBOLS, PROTOTYPES and version
    constant (`version_name`) are read now, not at import, and the library lands in its `_lib`.  dlopen, compare what `version_symbol`
    returns first -- a stale library may lack symbols the binding declares -- then require every exported symbol and declare the
    prototypes; those of `optional` only where the library has the symbol.  `label` names the version in the message."""
    path, rebuild = binding.LIB_PATH, "rebuild with `make -C nnop.jl_amd/csrc -j8`"
    if not os.path.exists(path):
        raise NNopLibraryMissing(
            f"{path} not found: build it with `make -C nnop.jl_amd/csrc -j8` "
            "(or __graft_entry__.build()).  There is no CPU or PyTorch fallback.")
    lib = C.CDLL(path)
    if not hasattr(lib, version_symbol):
        raise NNopLibraryMissing(f"{path} exports no {version_symbol}: {rebuild}")
    version, wanted = getattr(lib, version_symbol), getattr(binding, version_name)
    version.restype, version.argtypes = C.c_int, []
    if version() != wanted:
        raise NNopLibraryMissing(f"{path} has {label} {version()}, this binding needs {wanted}: {rebuild}")
    for name in binding.EXPORTED_SYMBOLS:
        if not hasattr(lib, name):
            raise NNopLibraryMissing(f"{path} does not export {name}: {rebuild}")
    prototypes = dict(binding.PROTOTYPES)
    prototypes.update((name, proto) for name, proto in (optional or {}).items() if hasattr(lib, name))
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    binding._lib = lib
    return lib


_lib = None


def load():
    """dlopen the library once and declare the prototypes.  Raises loudly when absent."""
    if _lib is not None:
        return _lib
    return load_library(sys.modules[__name__], "ABI version", "ABI_VERSION", "nnop_abi_version", optional=DEBUG_PROTOTYPES)


def strerror(status: int) -> str:
    return load().nnop_strerror(int(status)).decode()


def debug_set(key: str, value: int) -> int:
    """Test-only: override one launch-shape knob (csrc/tuning.hpp); -1 = automatic.  Returns the previous value.
    The hook is LOCKED unless the process environment held NNOP_DEBUG_HOOKS=1 at the library's first launch (the test-suite's
    conftest and bench.py set it): a production host cannot flip process-wide kernel selection by accident."""
    prev = load().nnop_debug_set(TUNE_KEYS[key], int(value))
    if prev == -(2 ** 31):
        if os.environ.get("NNOP_DEBUG_HOOKS", "0") in ("", "0"):
            raise RuntimeError("nnop_debug_set is locked: start the process with NNOP_DEBUG_HOOKS=1 (csrc/nnop_debug.h)")
        raise KeyError(key)
    return prev


def fa_shards(desc: FaDesc, world: int, rank: int):
    """nnop_fa_shards: rank's (batch, kv-head) unit range as <= 3 dense rectangles with their element offsets (host-only)."""
    out = (FaShard * 3)()
    n = load().nnop_fa_shards(C.byref(desc), int(world), int(rank), out)
    if n < 0:
        raise ValueError(strerror(n))
    return [out[i] for i in range(n)]


def dev_build() -> bool:
    return bool(load().nnop_debug_dev_build())


def fa_opts(window=None, desc=None):
    """FaOpts for a window (left, right) -- flash-attn's `window_size`, -1 = unbounded side -- or None for no options.
    With `desc`: also None when the window removes no key of that problem (the library's normalisation, FaWindow in
    csrc/fa_launch.hpp), so that such a call is the call without options in every respect -- the backward workspace included."""
    if window is None:
        return None
    if not isinstance(window, (tuple, list)) or len(window) != 2 or not all(isinstance(w, int) and not isinstance(w, bool)
                                                                           for w in window):
        raise TypeError(f"window must be None or a pair of ints (left, right), got {window!r}")
    left, right = int(window[0]), int(window[1])
    if desc is not None and left >= -1 and right >= -1:
        left_off = left == -1 or left >= desc.ql - 1
        right_off = right == -1 or right >= desc.kl - 1 or (desc.causal != 0 and right >= 0)
        if left_off and right_off:
            return None
    return FaOpts(window_left=left, window_right=right)


def fa_softcap(softcap=None):
    """Logit soft-capping as the library takes it: 0.0 for None / 0 (no cap: exactly the call without one), else the cap as a
    float.  A non-number is a TypeError; a negative or non-finite cap is refused by the library (NNOP_ERR_OPTS) -- and by
    attention.py before any GPU use."""
    if softcap is None:
        return 0.0
    if isinstance(softcap, bool) or not isinstance(softcap, numbers.Real):      # numpy's scalar types register as Real
        raise TypeError(f"softcap must be None or a number, got {softcap!r}")
    return float(softcap)


def fwd_form(desc: FaDesc, has_pair: bool = False, has_mask: bool = False, window=None, softcap=None) -> str:
    """Name of the forward kernel the launcher picks for this problem (reporting only; csrc/nnop_debug.h).  It names the form, not
    the symbol: a capped call launches the CAP = true instantiation of fa_fwd_kernel / fa_fwd_generic_kernel, a call with sinks the
    SINK = true instantiation of the form's kernel."""
    opts = fa_opts(window)
    if fa_softcap(softcap) != 0.0:
        code = load().nnop_debug_fwd_form_cap(C.byref(desc), C.byref(opts) if opts is not None else None, fa_softcap(softcap),
                                              int(has_pair), int(has_mask))
        if code >= 0:
            return FWD_FORMS_CAP[code]
    elif opts is None:
        code = load().nnop_debug_fwd_form(C.byref(desc), int(has_pair), int(has_mask))
    else:
        code = load().nnop_debug_fwd_form_ex(C.byref(desc), C.byref(opts), int(has_pair), int(has_mask))
    if code < 0:
        raise ValueError(strerror(code))
    return FWD_FORMS[code]


def bwd_kernels(desc: FaDesc, has_pair: bool = False, has_mask: bool = False, window=None, softcap=None):
    """Names of the (dK/dV, dQ) kernels the launcher picks for this problem (reporting only; csrc/nnop_debug.h).  It tells the w64
    backward from the fa_bwd.hpp one and no more: the plain-HIP kernels (fa_bwd_generic_*) report as the latter, and a capped call
    launches the same templates with the cap bit of MODE set (MODE 5, 6) or the CAP = true instantiations of the plain-HIP kernels."""
    opts = fa_opts(window)
    if fa_softcap(softcap) != 0.0:
        code = load().nnop_debug_bwd_form_cap(C.byref(desc), C.byref(opts) if opts is not None else None, fa_softcap(softcap),
                                              int(has_pair), int(has_mask))
    elif opts is None:
        code = load().nnop_debug_bwd_form(C.byref(desc), int(has_pair), int(has_mask))
    else:
        code = load().nnop_debug_bwd_form_ex(C.byref(desc), C.byref(opts), int(has_pair), int(has_mask))
    if code < 0:
        raise ValueError(strerror(code))
    return ("fa_bwd_w64_kernel<dK/dV>" if code & 1 else "fa_bwd_dkdv_kernel", "fa_bwd_w64_kernel<dQ>" if code & 2 else "fa_bwd_dq_kernel")
