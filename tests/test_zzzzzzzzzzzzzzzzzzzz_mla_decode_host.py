"""CPU tests of the C boundary and wrappers of MLA decode attention over a paged latent cache (include/nnop_hip_mla_decode.h): the
eighteenth library exports exactly its header's three functions and links none of the other seventeen, its descriptor matches the ctypes
one, the entry points validate in the header's order and return before any launch, the plan follows the header's rule, and the Python
wrappers raise before any device work.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from abi_util import ROOT, c_param_count, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_mla_decode.h")
NAMES = {"nnop_mla_decode_abi_version", "nnop_mla_decode_plan", "nnop_mla_decode"}
FIELDS = ["dtype", "ql", "qh", "batch", "max_pages", "page_size", "num_pages", "splits", "flags", "reserved0", "reserved1", "softmax_scale",
          "q_stride_b", "q_stride_h", "q_stride_l", "kv_stride_p", "kv_stride_l", "table_stride"]
# o lse q kv block_table seqlens workspace; the workspace is optional at one split
ALIGNS, OPTIONAL = (16, 4, 16, 16, 4, 4, 4), (1, 6)
OK, NULL = C.c_void_p(0x7f0000001000), C.c_void_p(0)         # never dereferenced: every call in this file returns before a launch
at = lambda off: C.c_void_p(0x7f0000001000 + off)


def test_library_header_and_binding_agree(pkg):
    M = pkg._lib_mla_decode
    lib = M.load()
    out = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = strip_c_comments(open(HEADER).read())
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == NAMES == set(M.EXPORTED_SYMBOLS)
    assert set(re.findall(r"\b(nnop_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert NAMES == set(re.findall(r"nnop_\w+(?=;)", open(os.path.join(ROOT, "nnop.jl_amd", "csrc", "nnop_mla_decode.map")).read()))
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes) and len(argtypes) == c_param_count(header.replace("(void)", "()"), name)
    assert lib.nnop_mla_decode_abi_version() == M.MLA_DECODE_ABI_VERSION == int(re.search(r"_ABI_VERSION (\d+)", header).group(1))
    assert "libnnop_hip" not in subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    body = re.search(r"typedef struct nnop_mla_decode_desc \{(.*?)\} nnop_mla_decode_desc;", header, re.S).group(1)
    names = [n.strip() for _, ns in re.findall(r"(u?int(?:32|64)_t|float)\s+([^;]+);", body) for n in ns.split(",")]
    D = M.MlaDecodeDesc
    assert names == FIELDS == [n for n, _ in D._fields_] and C.sizeof(D) == 96
    assert all(getattr(D, n).offset == 4 * i for i, n in enumerate(FIELDS[:12])) and all(getattr(D, n).offset == 48 + 8 * i for i, n in enumerate(FIELDS[12:]))
    assert (M.WIDTH, M.LATENT, M.MAX_HEADS, M.MAX_QL, M.MAX_SPLITS, M.MIN_PAGE_SIZE) == tuple(
        int(re.search(rf"#define NNOP_MLA_DECODE_{n}\s+(\d+)", header).group(1)) for n in ("WIDTH", "LATENT", "MAX_HEADS", "MAX_QL", "MAX_SPLITS", "MIN_PAGE_SIZE"))
    for name in ("mla_decode_attention", "mla_decode_attention_into", "mla_decode_attention_plan", "mla_decode", "_lib_mla_decode"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert pkg.mla_decode._ptr is pkg._common._ptr and pkg.mla_decode._raise is pkg._common._raise
    assert pkg.mla_decode._side is pkg.paged_prefill._side and pkg.mla_decode._strides is pkg.paged_prefill._strides


def _kw(**kw):
    base = dict(dtype=2, ql=1, qh=128, batch=4, max_pages=256, page_size=16, num_pages=1024, splits=0, flags=0, reserved0=0, reserved1=0,
                softmax_scale=192 ** -0.5, q_stride_b=128 * 576, q_stride_h=576, q_stride_l=576, kv_stride_p=16 * 576, kv_stride_l=576,
                table_stride=256)
    base.update(kw)
    return base


def _call(lib, d, ptrs, nbytes=1 << 40):
    return lib.nnop_mla_decode(C.byref(d), *ptrs, nbytes, None)


def _plan(lib, d):
    s, n = C.c_int32(-1), C.c_size_t(1)
    st = lib.nnop_mla_decode_plan(C.byref(d), C.byref(s), C.byref(n))
    return st, s.value, n.value


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=0), "NNOP_ERR_DTYPE"),                               # no fp32
    (dict(flags=1), "NNOP_ERR_OPTS"),
    (dict(reserved1=1), "NNOP_ERR_OPTS"),
    (dict(splits=65), "NNOP_ERR_OPTS"),
    (dict(softmax_scale=0.0), "NNOP_ERR_OPTS"),
    (dict(softmax_scale=float("inf")), "NNOP_ERR_OPTS"),
    (dict(softmax_scale=float("nan")), "NNOP_ERR_OPTS"),
    (dict(qh=24), "NNOP_ERR_SHAPE"),                                 # no multiple of 16
    (dict(qh=144), "NNOP_ERR_SHAPE"),
    (dict(ql=9), "NNOP_ERR_SHAPE"),
    (dict(ql=0), "NNOP_ERR_SHAPE"),
    (dict(page_size=8), "NNOP_ERR_SHAPE"),                           # a 16-key block would span two pages
    (dict(page_size=48), "NNOP_ERR_SHAPE"),                          # no power of two
    (dict(num_pages=0), "NNOP_ERR_SHAPE"),
    (dict(max_pages=2 ** 27), "NNOP_ERR_SHAPE"),                     # 2^31 keys
    (dict(kv_stride_l=512), "NNOP_ERR_SHAPE"),                       # below a row
    (dict(q_stride_l=580), "NNOP_ERR_SHAPE"),                        # no multiple of 8
    (dict(table_stride=255), "NNOP_ERR_SHAPE"),                      # below max_pages
    (dict(batch=2 ** 26, splits=64), "NNOP_ERR_SHAPE"),              # 2^33 workgroups
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=0, flags=1, page_size=8), "NNOP_ERR_DTYPE"),
    (dict(softmax_scale=-1.0, page_size=8), "NNOP_ERR_OPTS"),
])
def test_descriptor_checks_come_first_and_in_order(pkg, kw, status):
    M, want = pkg._lib_mla_decode, getattr(pkg._lib, status)
    lib, d = M.load(), M.MlaDecodeDesc(**_kw(**kw))
    for ptr in (OK, NULL, at(1)):
        assert _call(lib, d, [ptr] * 7) == want
    assert _plan(lib, d)[0] == want
    assert lib.nnop_mla_decode(None, *[OK] * 7, 0, None) == pkg._lib.NNOP_ERR_NULL == lib.nnop_mla_decode_plan(C.byref(d), None, None)


def test_null_alignment_and_workspace_checks_come_before_any_launch(pkg):
    M, L = pkg._lib_mla_decode, pkg._lib
    lib, d = M.load(), M.MlaDecodeDesc(**_kw(splits=4))              # a workspace is needed, so every pointer is judged
    need = _plan(lib, d)[2]
    assert need == 4 * 4 * 128 * 1 * 4 * 514
    for pos, a in enumerate(ALIGNS):
        b, c = [OK] * 7, [at(1)] * 7                                 # NULL is judged before alignment
        b[pos] = c[pos] = NULL
        assert _call(lib, d, c) == (L.NNOP_ERR_ALIGN if pos == 1 else L.NNOP_ERR_NULL), pos
        if pos != 1:
            assert _call(lib, d, b) == L.NNOP_ERR_NULL, pos
        c = [OK] * 7
        c[pos] = at(a // 2)                                          # aligned to half of what is needed
        assert _call(lib, d, c) == L.NNOP_ERR_ALIGN, pos
    assert _call(lib, d, [OK] * 7, need - 1) == L.NNOP_ERR_WORKSPACE
    one = M.MlaDecodeDesc(**_kw(splits=1))                           # one split: a NULL workspace of 0 bytes passes on to the alignment check
    assert _call(lib, one, [at(1)] * 6 + [NULL], 0) == L.NNOP_ERR_ALIGN and _call(lib, one, [NULL] * 7, 0) == L.NNOP_ERR_NULL


@pytest.mark.parametrize("kw,splits,nbytes", [
    # 1024 tiles, groups = 1 1 2: ceil(512 / 2) = 256 = 1024 / 4, capped at 64
    (dict(batch=1, max_pages=512, page_size=64, table_stride=512, kv_stride_p=64 * 576), 64, 4 * 128 * 64 * 514),
    # 10 tiles, groups = 8 2 1: ceil(512 / 16) = 32, but a chunk keeps 4 tiles: 10 / 4 = 2
    (dict(batch=8, qh=16, ql=2, max_pages=20, table_stride=20), 2, 4 * 8 * 16 * 2 * 2 * 514),
    # groups = 64 4 2 = 512: one split, no workspace
    (dict(batch=64, ql=4, max_pages=128, page_size=64, table_stride=128, kv_stride_p=64 * 576), 1, 0),
])
def test_the_plan_follows_the_headers_rule(pkg, kw, splits, nbytes):
    M = pkg._lib_mla_decode
    assert _plan(M.load(), M.MlaDecodeDesc(**_kw(**kw))) == (pkg._lib.NNOP_OK, splits, nbytes)
    assert _plan(M.load(), M.MlaDecodeDesc(**_kw(splits=7, **kw)))[1] == 7


class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt).as_subclass(OnGpu)
    q, kv, tab, lens = mk(2, 32, 2, 576), mk(9, 16, 576), mk(2, 3, dt=torch.int32), mk(2, dt=torch.int32)
    A, E = pkg.mla_decode_attention, pkg.NNopError
    with pytest.raises(E, match="GPU-only"):
        A(q, kv, torch.zeros(2, 3, dtype=torch.int32), lens)
    for bad, status in ((lambda: A(mk(2, 32, 2, 576, dt=torch.float32), kv, tab, lens), "NNOP_ERR_DTYPE"),
                        (lambda: A(q, mk(9, 16, 576, dt=torch.float16), tab, lens), "NNOP_ERR_DTYPE"),
                        (lambda: A(q, kv, mk(2, 3, dt=torch.int64), lens), "NNOP_ERR_DTYPE"),           # the table's dtype
                        (lambda: A(mk(2, 24, 2, 576), kv, tab, lens), "NNOP_ERR_SHAPE"),                # QH = 24, 144
                        (lambda: A(mk(2, 144, 2, 576), kv, tab, lens), "NNOP_ERR_SHAPE"),
                        (lambda: A(mk(2, 32, 9, 576), kv, tab, lens), "NNOP_ERR_SHAPE"),                # QL = 9
                        (lambda: A(mk(2, 32, 2, 512), kv, tab, lens), "NNOP_ERR_SHAPE"),                # the latent part alone
                        (lambda: A(q, mk(9, 8, 576), tab, lens), "NNOP_ERR_SHAPE"),                     # page sizes 8 and 48
                        (lambda: A(q, mk(9, 48, 576), tab, lens), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, kv, tab, mk(3, dt=torch.int32)), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, kv, tab, lens, softmax_scale=0.0), "NNOP_ERR_OPTS"),
                        (lambda: A(q, kv, tab, lens, softmax_scale=-0.1), "NNOP_ERR_OPTS"),
                        (lambda: A(q, kv, tab, lens, softmax_scale=float("inf")), "NNOP_ERR_OPTS"),
                        (lambda: A(q, kv, tab, lens, softmax_scale=float("nan")), "NNOP_ERR_OPTS")):
        with pytest.raises(E) as e:
            bad()
        assert e.value.status == getattr(pkg._lib, status)
    with pytest.raises(ValueError):
        A(q, kv, tab, lens, num_splits=65)
    # a transposed q, a [P, page, 1, 576] pool and a slice of a larger table become strides, never a copy; the plan needs no device
    pool4 = mk(9, 16, 1, 584)[..., :576]
    view, d = pkg.mla_decode._desc(mk(2, 2, 32, 576).transpose(1, 2), pool4, mk(2, 8, dt=torch.int32)[:, 2:5], 0.1, 3)
    assert view.data_ptr() == pool4.data_ptr() and view.shape == (9, 16, 576)
    assert (d.q_stride_b, d.q_stride_h, d.q_stride_l, d.kv_stride_p, d.kv_stride_l, d.table_stride) == (2 * 32 * 576, 576, 32 * 576, 16 * 584, 584, 8)
    assert (d.ql, d.qh, d.batch, d.max_pages, d.page_size, d.num_pages, d.splits, d.softmax_scale) == (2, 32, 2, 3, 16, 9, 3, C.c_float(0.1).value)
    assert pkg.mla_decode._desc(q, kv, tab, None, None)[1].softmax_scale == C.c_float(192 ** -0.5).value
    assert pkg.mla_decode_attention_plan(q, kv, tab, num_splits=3) == (3, 4 * 2 * 32 * 2 * 3 * 514)
    assert pkg.mla_decode_attention_plan(q, kv, tab) == (1, 0)
