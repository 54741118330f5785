"""CPU tests of the C boundary and wrappers of decode attention over an E4M3 cache (include/nnop_hip_decode_attn_fp8.h): the eleventh
library exports exactly its header's three functions and links none of the other ten, its descriptor matches the ctypes one and the
tenth library's layout, the entry points validate in the header's order and return before any launch, the plan is the tenth library's,
and the Python wrappers raise before any device work.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from abi_util import ROOT, c_param_count, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_decode_attn_fp8.h")
NAMES = {"nnop_decode_attn_fp8_abi_version", "nnop_decode_attn_fp8_plan", "nnop_decode_attn_fp8"}
FIELDS = ["dtype", "emb", "ql", "qh", "kh", "batch", "capacity", "window_left", "splits", "flags", "kv_format", "reserved",
          "k_stride_b", "k_stride_h", "k_stride_l", "v_stride_b", "v_stride_h", "v_stride_l"]
# o lse q k v k_scale v_scale seqlens sinks workspace; the workspace is optional at one split
ALIGNS, OPTIONAL = (16, 4, 16, 16, 16, 4, 4, 4, 4, 4), (1, 5, 6, 8, 9)
OK, NULL = C.c_void_p(0x7f0000001000), C.c_void_p(0)         # never dereferenced: every call in this file returns before a launch
at = lambda off: C.c_void_p(0x7f0000001000 + off)


def test_library_header_and_binding_agree(pkg):
    M = pkg._lib_decode_attn_fp8
    lib = M.load()
    out = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = strip_c_comments(open(HEADER).read())
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == NAMES == set(M.EXPORTED_SYMBOLS)
    assert set(re.findall(r"\b(nnop_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert NAMES == set(re.findall(r"nnop_\w+(?=;)", open(os.path.join(ROOT, "nnop.jl_amd", "csrc", "nnop_decode_attn_fp8.map")).read()))
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes) and len(argtypes) == c_param_count(header.replace("(void)", "()"), name)
    assert lib.nnop_decode_attn_fp8_abi_version() == M.DECODE_ATTN_FP8_ABI_VERSION == int(re.search(r"_ABI_VERSION (\d+)", header).group(1))
    assert "libnnop_hip" not in subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    body = re.search(r"typedef struct nnop_decode_attn_fp8_desc \{(.*?)\} nnop_decode_attn_fp8_desc;", header, re.S).group(1)
    names = [re.match(r"\w+", n.strip()).group(0) for _, ns in re.findall(r"(u?int(?:32|64)_t)\s+([^;]+);", body) for n in ns.split(",")]
    D, D16 = M.DecodeAttnFp8Desc, pkg._lib_decode_attn.DecodeAttnDesc
    assert names == FIELDS == [n for n, _ in D._fields_] and C.sizeof(D) == C.sizeof(D16) == 96
    assert D.kv_format.offset == D16.reserved.offset and all(getattr(D, n).offset == getattr(D16, n).offset for n in FIELDS[:10] + FIELDS[12:])
    assert (M.MAX_ROWS, M.MAX_SPLITS, M.KV_E4M3) == tuple(int(re.search(rf"#define NNOP_DECODE_ATTN_FP8_{n}\s+(\d+)", header).group(1))
                                                          for n in ("MAX_ROWS", "MAX_SPLITS", "E4M3"))
    for name in ("decode_attention_fp8", "decode_attention_fp8_into", "decode_attention_fp8_plan", "decode_attn_fp8", "_lib_decode_attn_fp8"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert pkg.decode_attn_fp8._ptr is pkg._common._ptr and pkg.decode_attn_fp8._raise is pkg._common._raise


def _kw(**kw):
    base = dict(dtype=2, emb=64, ql=1, qh=64, kh=8, batch=4, capacity=4096, window_left=-1, splits=0, flags=0)
    base.update({f"{t}_stride_{a}": s for t in "kv" for a, s in (("b", 8 * 4096 * 64), ("h", 4096 * 64), ("l", 64))})
    base.update(kw)
    return base


def _call(lib, d, ptrs, nbytes=1 << 40):
    return lib.nnop_decode_attn_fp8(C.byref(d), *ptrs, nbytes, None)


def _plan(lib, fn, d):
    s, n = C.c_int32(-1), C.c_size_t(1)
    st = getattr(lib, fn)(C.byref(d), C.byref(s), C.byref(n))
    return st, s.value, n.value


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=0), "NNOP_ERR_DTYPE"),                               # no fp32
    (dict(flags=1), "NNOP_ERR_OPTS"),
    (dict(kv_format=1), "NNOP_ERR_OPTS"),                            # E5M2 is not built
    (dict(reserved=5), "NNOP_ERR_OPTS"),
    (dict(window_left=-2), "NNOP_ERR_OPTS"),
    (dict(splits=65), "NNOP_ERR_OPTS"),
    (dict(emb=32), "NNOP_ERR_SHAPE"),
    (dict(qh=136), "NNOP_ERR_SHAPE"),                                # G = 17
    (dict(ql=3), "NNOP_ERR_SHAPE"),                                  # G QL = 24
    (dict(qh=8, ql=2, capacity=1), "NNOP_ERR_SHAPE"),                # the cache cannot hold the new tokens
    (dict(k_stride_l=24), "NNOP_ERR_SHAPE"),                         # below a row
    (dict(v_stride_h=4096 * 64 + 24), "NNOP_ERR_SHAPE"),             # a multiple of 8, which the 16-bit call takes, but not of 16
    (dict(batch=2 ** 26, splits=8), "NNOP_ERR_SHAPE"),               # 2^32 workgroups
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=0, kv_format=1, emb=32), "NNOP_ERR_DTYPE"),
    (dict(kv_format=1, emb=32), "NNOP_ERR_OPTS"),
])
def test_descriptor_checks_come_first_and_in_order(pkg, kw, status):
    M, want = pkg._lib_decode_attn_fp8, getattr(pkg._lib, status)
    lib, d = M.load(), M.DecodeAttnFp8Desc(**_kw(**kw))
    for ptr in (OK, NULL, at(1)):
        assert _call(lib, d, [ptr] * 10) == want
    assert _plan(lib, "nnop_decode_attn_fp8_plan", d)[0] == want
    assert lib.nnop_decode_attn_fp8(None, *[OK] * 10, 0, None) == pkg._lib.NNOP_ERR_NULL == lib.nnop_decode_attn_fp8_plan(C.byref(d), None, None)


def test_null_alignment_and_workspace_checks_come_before_any_launch(pkg):
    M, L = pkg._lib_decode_attn_fp8, pkg._lib
    lib, d = M.load(), M.DecodeAttnFp8Desc(**_kw(splits=4))          # a workspace is needed, so every pointer is judged
    need = _plan(lib, "nnop_decode_attn_fp8_plan", d)[2]
    assert need == 4 * 4 * 64 * 1 * 4 * 66
    for pos, a in enumerate(ALIGNS):
        b, c = [OK] * 10, [at(1)] * 10                               # NULL is judged before alignment
        b[pos] = c[pos] = NULL
        assert _call(lib, d, c) == (L.NNOP_ERR_ALIGN if pos in OPTIONAL[:4] else L.NNOP_ERR_NULL), pos
        if pos not in OPTIONAL[:4]:
            assert _call(lib, d, b) == L.NNOP_ERR_NULL, pos
        c = [OK] * 10
        c[pos] = at(a // 2)                                          # aligned to half of what is needed: an unaligned scale among them
        assert _call(lib, d, c) == L.NNOP_ERR_ALIGN, pos
    assert _call(lib, d, [OK] * 10, need - 1) == L.NNOP_ERR_WORKSPACE
    one = M.DecodeAttnFp8Desc(**_kw(splits=1))                       # one split: a NULL workspace of 0 bytes passes on to the alignment check
    assert _call(lib, one, [at(1)] * 9 + [NULL], 0) == L.NNOP_ERR_ALIGN and _call(lib, one, [NULL] * 10, 0) == L.NNOP_ERR_NULL


@pytest.mark.parametrize("kw", [dict(batch=1, capacity=65536), dict(batch=8, capacity=8192), dict(batch=64), dict(batch=1, capacity=300),
                                dict(batch=1, capacity=65536, window_left=128), dict(batch=1, capacity=100, splits=7),
                                dict(batch=1, emb=128, splits=2, k_stride_l=128, v_stride_l=128), dict(qh=8, ql=2, window_left=1000)])
def test_the_plan_is_the_tenth_librarys(pkg, kw):
    M8, M16 = pkg._lib_decode_attn_fp8, pkg._lib_decode_attn
    got = _plan(M8.load(), "nnop_decode_attn_fp8_plan", M8.DecodeAttnFp8Desc(**_kw(**kw)))
    assert got[0] == pkg._lib.NNOP_OK and got == _plan(M16.load(), "nnop_decode_attn_plan", M16.DecodeAttnDesc(**_kw(**kw)))


class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt).as_subclass(OnGpu)
    f8 = lambda *s: mk(*s, dt=torch.uint8).view(torch.float8_e4m3fn)
    q, k, v, lens = mk(2, 16, 1, 64), f8(2, 2, 48, 64), mk(2, 2, 48, 64, dt=torch.uint8), mk(2, dt=torch.int32)
    A, E = pkg.decode_attention_fp8, pkg.NNopError
    with pytest.raises(E, match="GPU-only"):
        A(q, torch.zeros(2, 2, 48, 64, dtype=torch.uint8), v, lens)
    with pytest.raises(E, match="flash_attention"):
        A(mk(2, 16, 1, 64, dt=torch.float32).requires_grad_(True).to(torch.bfloat16).as_subclass(OnGpu), k, v, lens)
    for bad, status in ((lambda: A(q, mk(2, 2, 48, 64), v, lens), "NNOP_ERR_DTYPE"),               # a bf16 cache is decode_attention's
                        (lambda: A(mk(2, 16, 1, 64, dt=torch.float32), k, v, lens), "NNOP_ERR_DTYPE"),
                        (lambda: A(q, k, v, lens, k_scale=mk(3, dt=torch.float32)), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, k, v, lens, v_scale=mk(2, dt=torch.bfloat16)), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, f8(2, 2, 48, 72)[..., :64], v, lens), "NNOP_ERR_SHAPE"),     # a row stride of 72: no multiple of 16
                        (lambda: A(mk(2, 34, 1, 64), k, v, lens), "NNOP_ERR_SHAPE"),               # G = 17
                        (lambda: A(q, k, v, mk(3, dt=torch.int32)), "NNOP_ERR_SHAPE")):
        with pytest.raises(E) as e:
            bad()
        assert e.value.status == getattr(pkg._lib, status)
    with pytest.raises(ValueError):
        A(q, k, v, lens, num_splits=65)
    # both cache layouts become byte strides, never a copy; the plan needs no device
    d = pkg.decode_attn_fp8._desc(q, f8(2, 48, 2, 64).transpose(1, 2), v, 128, 3)
    assert (d.k_stride_b, d.k_stride_h, d.k_stride_l, d.v_stride_b, d.v_stride_h, d.v_stride_l) == (6144, 64, 128, 6144, 3072, 64)
    assert (d.window_left, d.splits, d.capacity, d.qh, d.kh, d.kv_format, d.reserved) == (48, 3, 48, 16, 2, 0, 0)
    assert pkg.decode_attention_fp8_plan(q, k, v, num_splits=3) == (3, 4 * 2 * 16 * 3 * 66) and pkg.decode_attention_fp8_plan(q, k, v) == (1, 0)
