"""Shared helpers of the CPU tests of the C ABI (include/nnop_hip.h) and of the Julia shim (test infrastructure, not a test file)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nnop_hip.h")
SHIM = os.path.join(ROOT, "nnop.jl_amd", "julia", "NNopHIPExt.jl")


def fa_desc(pkg, **kw):
    """a valid attention descriptor (bf16 E64 128 x 128 H4 B2) with `kw` on top"""
    base = dict(dtype=pkg._lib.NNOP_BF16, emb=64, ql=128, kl=128, qh=4, kh=4, batch=2, causal=0)
    base.update(kw)
    return pkg._lib.FaDesc(**base)


def fa_opts(pkg, left=-1, right=-1, reserved=None):
    o = pkg._lib.FaOpts(window_left=left, window_right=right)
    for i, r in enumerate(reserved or []):
        o.reserved[i] = r
    return o


def strip_c_comments(src):
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def c_params(header, name):
    """the parameter declarations of the prototype of `name` in the (comment-free) header"""
    proto = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
    return [p.strip() for p in proto.split(",") if p.strip()]


def c_param_count(header, name):
    return len(c_params(header, name))


def jl_ccall_types(shim, name):
    """the argument type tuple of the shim's ccall of `name`"""
    shim = re.sub(r"#[^\n]*", "", shim)
    m = re.search(r"ccall\(\(:" + name + r", libnnop\(\)\), Cint,\s*\((.*?)\),\s*\n\s*d,", shim, re.S)
    assert m, name
    return [t.strip() for t in m.group(1).split(",") if t.strip()]
