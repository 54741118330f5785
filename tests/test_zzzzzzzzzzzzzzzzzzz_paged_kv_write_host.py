"""CPU tests of the C boundary and wrapper of the paged KV-cache write (include/nnop_hip_paged_kv_write.h): the seventeenth library exports
exactly its header's two functions and links none of the other sixteen, its descriptor matches the ctypes one, the entry point validates
in the header's order and returns before any launch, and the Python wrapper raises before any device work.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from abi_util import ROOT, c_param_count, strip_c_comments
from test_zzzzzzzzzzzzzzz_paged_prefill_host import NULL, OK, OnGpu, at

HEADER = os.path.join(ROOT, "include", "nnop_hip_paged_kv_write.h")
NAMES = {"nnop_paged_kv_write_abi_version", "nnop_paged_kv_write"}
FIELDS = ["dtype", "emb", "tokens", "kh", "batch", "max_pages", "page_size", "num_pages", "kv_format", "reserved", "flags", "reserved2",
          "kp_stride_p", "kp_stride_h", "kp_stride_l", "vp_stride_p", "vp_stride_h", "vp_stride_l", "table_stride",
          "k_stride_t", "k_stride_h", "v_stride_t", "v_stride_h"]
# k_pages v_pages k v k_scale v_scale block_table cu_seqlens_q seqlens; the scales are optional
ALIGNS, OPTIONAL = (16, 16, 16, 16, 4, 4, 4, 4, 4), (4, 5)


def test_library_header_and_binding_agree(pkg):
    M = pkg._lib_paged_kv_write
    lib = M.load()
    out = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = strip_c_comments(open(HEADER).read())
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == NAMES == set(M.EXPORTED_SYMBOLS)
    assert set(re.findall(r"\b(nnop_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert NAMES == set(re.findall(r"nnop_\w+(?=;)", open(os.path.join(ROOT, "nnop.jl_amd", "csrc", "nnop_paged_kv_write.map")).read()))
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes) and len(argtypes) == c_param_count(header.replace("(void)", "()"), name)
    assert lib.nnop_paged_kv_write_abi_version() == M.PAGED_KV_WRITE_ABI_VERSION == int(re.search(r"_ABI_VERSION (\d+)", header).group(1))
    assert "libnnop_hip" not in subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    body = re.search(r"typedef struct nnop_paged_kv_write_desc \{(.*?)\} nnop_paged_kv_write_desc;", header, re.S).group(1)
    names = [re.match(r"\w+", n.strip()).group(0) for _, ns in re.findall(r"(u?int(?:32|64)_t)\s+([^;]+);", body) for n in ns.split(",")]
    D = M.PagedKvWriteDesc
    assert names == FIELDS == [n for n, _ in D._fields_] and C.sizeof(D) == 136
    assert all(getattr(D, n).offset == 4 * i for i, n in enumerate(FIELDS[:12])) and all(getattr(D, n).offset == 48 + 8 * i for i, n in enumerate(FIELDS[12:]))
    assert (M.BLOCK_TOKENS, M.MIN_PAGE_SIZE, M.KV_16BIT, M.KV_E4M3) == tuple(
        int(re.search(rf"#define NNOP_PAGED_KV_WRITE_{n}\s+(\d+)", header).group(1)) for n in ("BLOCK_TOKENS", "MIN_PAGE_SIZE", "16BIT", "E4M3"))
    for name in ("paged_kv_cache_write", "paged_kv_write", "_lib_paged_kv_write"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert pkg.paged_kv_write._tensor is pkg.paged_prefill._tensor and pkg.paged_kv_write._side is pkg.paged_prefill._side


def _kw(**kw):
    base = dict(dtype=2, emb=64, tokens=1000, kh=8, batch=4, max_pages=256, page_size=16, num_pages=1024, kv_format=1, reserved=0, flags=0,
                reserved2=0, table_stride=256, k_stride_t=8 * 64, k_stride_h=64, v_stride_t=8 * 64, v_stride_h=64)
    base.update({f"{t}p_stride_{a}": s for t in "kv" for a, s in (("p", 8 * 16 * 64), ("h", 16 * 64), ("l", 64))})
    base.update(kw)
    return base


def _call(lib, d, ptrs):
    return lib.nnop_paged_kv_write(C.byref(d), *ptrs, None)


@pytest.mark.parametrize("kw,status,scales", [
    (dict(dtype=0), "NNOP_ERR_DTYPE", OK),                           # no fp32
    (dict(flags=1), "NNOP_ERR_OPTS", OK),
    (dict(reserved=1), "NNOP_ERR_OPTS", OK),
    (dict(reserved2=1), "NNOP_ERR_OPTS", OK),
    (dict(kv_format=2), "NNOP_ERR_OPTS", OK),                        # E5M2 is not there
    (dict(kv_format=0), "NNOP_ERR_OPTS", OK),                        # scales with a 16-bit pool
    (dict(emb=32), "NNOP_ERR_SHAPE", OK),
    (dict(tokens=0), "NNOP_ERR_SHAPE", OK),
    (dict(kh=0), "NNOP_ERR_SHAPE", OK),
    (dict(kh=2 ** 25, k_stride_t=2 ** 31, v_stride_t=2 ** 31), "NNOP_ERR_SHAPE", OK),   # 2^31 elements a row
    (dict(page_size=8), "NNOP_ERR_SHAPE", OK),
    (dict(page_size=48), "NNOP_ERR_SHAPE", OK),                      # no power of two
    (dict(num_pages=0), "NNOP_ERR_SHAPE", OK),
    (dict(max_pages=2 ** 27), "NNOP_ERR_SHAPE", OK),                 # 2^31 keys
    (dict(kp_stride_l=48), "NNOP_ERR_SHAPE", OK),                    # below a row
    (dict(vp_stride_p=8 * 16 * 64 + 8), "NNOP_ERR_SHAPE", OK),       # E4M3: 8 bytes are no multiple of 16 ...
    (dict(k_stride_h=68), "NNOP_ERR_SHAPE", OK),
    (dict(v_stride_t=8 * 64 - 8), "NNOP_ERR_SHAPE", OK),             # tokens of v overlap
    (dict(table_stride=255), "NNOP_ERR_SHAPE", OK),                  # below max_pages
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=0, kv_format=0, page_size=8), "NNOP_ERR_DTYPE", OK),
    (dict(kv_format=0, page_size=8), "NNOP_ERR_OPTS", OK),
    (dict(flags=1, page_size=8), "NNOP_ERR_OPTS", NULL),
])
def test_descriptor_checks_come_first_and_in_order(pkg, kw, status, scales):
    M, want = pkg._lib_paged_kv_write, getattr(pkg._lib, status)
    lib, d = M.load(), M.PagedKvWriteDesc(**_kw(**kw))
    for ptr in (OK, NULL, at(1)):
        assert _call(lib, d, [ptr] * 4 + [scales] * 2 + [ptr] * 3) == want
    assert lib.nnop_paged_kv_write(None, *[OK] * 9, None) == pkg._lib.NNOP_ERR_NULL


def test_null_and_alignment_checks_come_before_any_launch(pkg):
    M, L = pkg._lib_paged_kv_write, pkg._lib
    lib, d = M.load(), M.PagedKvWriteDesc(**_kw())
    # a 16-bit pool without scales is no option error, and 8 of its elements are 16 bytes: the pointer check answers
    assert _call(lib, M.PagedKvWriteDesc(**_kw(kv_format=0, vp_stride_p=8 * 16 * 64 + 8)), [NULL] * 9) == L.NNOP_ERR_NULL
    assert _call(lib, M.PagedKvWriteDesc(**_kw(kv_format=0, vp_stride_p=8 * 16 * 64 + 4)), [NULL] * 9) == L.NNOP_ERR_SHAPE
    for pos, a in enumerate(ALIGNS):
        b, c = [OK] * 9, [at(1)] * 9                                 # NULL is judged before alignment
        b[pos] = c[pos] = NULL
        assert _call(lib, d, c) == (L.NNOP_ERR_ALIGN if pos in OPTIONAL else L.NNOP_ERR_NULL), pos
        if pos not in OPTIONAL:
            assert _call(lib, d, b) == L.NNOP_ERR_NULL, pos
        c = [OK] * 9
        c[pos] = at(a // 2)                                          # aligned to half of what is needed
        assert _call(lib, d, c) == L.NNOP_ERR_ALIGN, pos


def test_python_checks_raise_before_device_work(pkg):
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt).as_subclass(OnGpu)
    k, v, kp, vp, tab = mk(7, 2, 64), mk(7, 2, 64), mk(9, 2, 16, 64), mk(9, 2, 16, 64), mk(2, 3, dt=torch.int32)
    k8, v8 = mk(9, 2, 16, 64, dt=torch.float8_e4m3fn), mk(9, 2, 16, 64, dt=torch.uint8)
    cu, lens, sc = mk(3, dt=torch.int32), mk(2, dt=torch.int32), mk(2, dt=torch.float32)
    W, E = pkg.paged_kv_cache_write, pkg.NNopError
    with pytest.raises(E, match="GPU-only"):
        W(k, v, kp, torch.zeros(9, 2, 16, 64, dtype=torch.bfloat16), tab, cu, lens)                       # devices
    for bad, status in ((lambda: W(mk(7, 2, 64, dt=torch.float32), v, kp, vp, tab, cu, lens), "NNOP_ERR_DTYPE"),
                        (lambda: W(k, mk(7, 2, 64, dt=torch.float16), kp, vp, tab, cu, lens), "NNOP_ERR_DTYPE"),
                        (lambda: W(k, v, mk(9, 2, 16, 64, dt=torch.float16), vp, tab, cu, lens), "NNOP_ERR_DTYPE"),   # a 16-bit pool of another dtype
                        (lambda: W(k, v, k8, vp, tab, cu, lens), "NNOP_ERR_DTYPE"),                       # two formats
                        (lambda: W(k, v, kp, vp, tab.long().as_subclass(OnGpu), cu, lens), "NNOP_ERR_DTYPE"),
                        (lambda: W(k, v, kp, vp, tab, cu, lens, k_scale=sc), "NNOP_ERR_OPTS"),            # scales with a 16-bit pool
                        (lambda: W(k, v, kp, vp, tab, cu, lens, v_scale=sc), "NNOP_ERR_OPTS"),
                        (lambda: W(k, mk(7, 1, 64), kp, vp, tab, cu, lens), "NNOP_ERR_SHAPE"),
                        (lambda: W(k, v, mk(9, 3, 16, 64), mk(9, 3, 16, 64), tab, cu, lens), "NNOP_ERR_SHAPE"),   # KH of the pools
                        (lambda: W(k, v, mk(9, 2, 8, 64), mk(9, 2, 8, 64), tab, cu, lens), "NNOP_ERR_SHAPE"),
                        (lambda: W(mk(7, 2, 68)[..., :64], v, kp, vp, tab, cu, lens), "NNOP_ERR_SHAPE"),  # a head stride of 68
                        (lambda: W(k, v, k8, mk(9, 2, 16, 72, dt=torch.uint8)[..., :64], tab, cu, lens), "NNOP_ERR_SHAPE"),   # 72 bytes: no multiple of 16
                        (lambda: W(k, v, kp, vp, tab, mk(2, dt=torch.int32), lens), "NNOP_ERR_SHAPE"),    # cu_seqlens_q is [B + 1]
                        (lambda: W(k, v, kp, vp, tab, cu, mk(3, dt=torch.int32)), "NNOP_ERR_SHAPE"),
                        (lambda: W(k, v, kp, vp, tab, cu.long().as_subclass(OnGpu), lens), "NNOP_ERR_SHAPE"),
                        (lambda: W(k, v, k8, v8, tab, cu, lens, k_scale=mk(3, dt=torch.float32)), "NNOP_ERR_SHAPE")):
        with pytest.raises(E) as e:
            bad()
        assert e.value.status == getattr(pkg._lib, status)
    # slices of a fused projection, both pool layouts and both code dtypes become strides and a format, never a copy; no token, no launch
    qkv = mk(7, (4 + 2 * 2) * 64)
    d = pkg.paged_kv_write._desc(qkv[:, 256:384].view(7, 2, 64), qkv[:, 384:].view(7, 2, 64), k8, mk(9, 16, 2, 64, dt=torch.uint8).transpose(1, 2),
                                 mk(2, 8, dt=torch.int32)[:, 2:5], scales=True)
    assert (d.k_stride_t, d.k_stride_h, d.v_stride_t, d.v_stride_h, d.tokens, d.kh, d.batch) == (512, 64, 512, 64, 7, 2, 2)
    assert (d.kp_stride_p, d.kp_stride_h, d.kp_stride_l, d.vp_stride_p, d.vp_stride_h, d.vp_stride_l, d.table_stride) == (2048, 1024, 64, 2048, 64, 128, 8)
    assert (d.kv_format, d.max_pages, d.page_size, d.num_pages) == (pkg._lib_paged_kv_write.KV_E4M3, 3, 16, 9)
    assert pkg.paged_kv_write._desc(k, v, kp, vp, tab).kv_format == pkg._lib_paged_kv_write.KV_16BIT
    assert W(k[:0], v[:0], kp, vp, tab, cu, lens) is None
