"""CPU tests of decode attention's C boundary and wrappers (include/nnop_hip_decode_attn.h): the tenth library exports exactly its header's
three functions and links none of the other nine, its descriptor matches the ctypes one, the entry points validate in the header's order
and return before any launch, the plan follows the header's rule, and the Python wrappers raise before any device work.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from abi_util import ROOT, c_param_count, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_decode_attn.h")
NAMES = {"nnop_decode_attn_abi_version", "nnop_decode_attn_plan", "nnop_decode_attn"}
FIELDS = ["dtype", "emb", "ql", "qh", "kh", "batch", "capacity", "window_left", "splits", "flags", "reserved",
          "k_stride_b", "k_stride_h", "k_stride_l", "v_stride_b", "v_stride_h", "v_stride_l"]
ALIGNS, OPTIONAL = (16, 4, 16, 16, 16, 4, 4, 4), (1, 6, 7)   # o lse q k v seqlens sinks workspace; the workspace is optional at one split
OK, NULL = C.c_void_p(0x7f0000001000), C.c_void_p(0)         # never dereferenced: every call in this file returns before a launch
at = lambda off: C.c_void_p(0x7f0000001000 + off)


def test_library_header_and_binding_agree(pkg):
    M = pkg._lib_decode_attn
    lib = M.load()
    out = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = strip_c_comments(open(HEADER).read())
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == NAMES == set(M.EXPORTED_SYMBOLS)
    assert set(re.findall(r"\b(nnop_[a-z0-9_]+)\s*\(", header)) == NAMES
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes) and len(argtypes) == c_param_count(header.replace("(void)", "()"), name)
    assert lib.nnop_decode_attn_abi_version() == M.DECODE_ATTN_ABI_VERSION == int(re.search(r"_ABI_VERSION (\d+)", header).group(1))
    assert "libnnop_hip" not in subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    body = re.search(r"typedef struct nnop_decode_attn_desc \{(.*?)\} nnop_decode_attn_desc;", header, re.S).group(1)
    names = [re.match(r"\w+", n.strip()).group(0) for _, ns in re.findall(r"(u?int(?:32|64)_t)\s+([^;]+);", body) for n in ns.split(",")]
    D = M.DecodeAttnDesc
    assert names == FIELDS == [n for n, _ in D._fields_] and C.sizeof(D) == 96 and D.k_stride_b.offset == 48
    assert (M.MAX_ROWS, M.MAX_SPLITS) == tuple(int(re.search(rf"#define NNOP_DECODE_ATTN_{n}\s+(\d+)", header).group(1))
                                               for n in ("MAX_ROWS", "MAX_SPLITS"))
    for name in ("decode_attention", "decode_attention_into", "decode_attention_plan", "decode_attn", "_lib_decode_attn"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert pkg.decode_attn._ptr is pkg._common._ptr and pkg.decode_attn._raise is pkg._common._raise


def _desc(pkg, reserved=(0, 0), **kw):
    base = dict(dtype=2, emb=64, ql=1, qh=64, kh=8, batch=4, capacity=4096, window_left=-1, splits=0, flags=0)
    base.update({f"{t}_stride_{a}": s for t in "kv" for a, s in (("b", 8 * 4096 * 64), ("h", 4096 * 64), ("l", 64))})
    base.update(kw)
    d = pkg._lib_decode_attn.DecodeAttnDesc(**base)
    d.reserved[0], d.reserved[1] = reserved
    return d


def _call(lib, d, ptrs, nbytes=1 << 40):
    return lib.nnop_decode_attn(C.byref(d) if d is not None else None, *ptrs, nbytes, None)


def _plan(pkg, d):
    s, n = C.c_int32(-1), C.c_size_t(1)
    st = pkg._lib_decode_attn.load().nnop_decode_attn_plan(C.byref(d), C.byref(s), C.byref(n))
    return st, s.value, n.value


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=0), "NNOP_ERR_DTYPE"),                               # no fp32
    (dict(dtype=9), "NNOP_ERR_DTYPE"),
    (dict(flags=1), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, 5)), "NNOP_ERR_OPTS"),
    (dict(window_left=-2), "NNOP_ERR_OPTS"),
    (dict(splits=-1), "NNOP_ERR_OPTS"),
    (dict(splits=65), "NNOP_ERR_OPTS"),
    (dict(emb=32), "NNOP_ERR_SHAPE"),
    (dict(emb=256), "NNOP_ERR_SHAPE"),
    (dict(qh=60), "NNOP_ERR_SHAPE"),                                 # QH % KH
    (dict(qh=136), "NNOP_ERR_SHAPE"),                                # G = 17
    (dict(ql=3), "NNOP_ERR_SHAPE"),                                  # G QL = 24
    (dict(ql=0), "NNOP_ERR_SHAPE"),
    (dict(batch=0), "NNOP_ERR_SHAPE"),
    (dict(qh=8, ql=2, capacity=1), "NNOP_ERR_SHAPE"),                # the cache cannot hold the new tokens
    (dict(k_stride_l=56), "NNOP_ERR_SHAPE"),                         # below a row
    (dict(v_stride_h=4096 * 64 + 4), "NNOP_ERR_SHAPE"),              # no multiple of 8 elements
    (dict(batch=2 ** 26, splits=8), "NNOP_ERR_SHAPE"),               # 2^32 workgroups
    (dict(batch=2 ** 26), "NNOP_ERR_SHAPE"),                         # 2^29 workgroups, but 2^32 rows of o for the merge's grid
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=0, flags=1, emb=32), "NNOP_ERR_DTYPE"),
    (dict(splits=-1, emb=32), "NNOP_ERR_OPTS"),
])
def test_descriptor_checks_come_first_and_in_order(pkg, kw, status):
    lib, want = pkg._lib_decode_attn.load(), getattr(pkg._lib, status)
    d = _desc(pkg, **kw)
    for ptr in (OK, NULL, at(1)):
        assert _call(lib, d, [ptr] * 8) == want
    assert _plan(pkg, d)[0] == want
    assert _call(lib, None, [OK] * 8) == pkg._lib.NNOP_ERR_NULL == lib.nnop_decode_attn_plan(C.byref(d), None, None)


def test_null_alignment_and_workspace_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib_decode_attn.load(), pkg._lib
    d = _desc(pkg, splits=4)                                         # a workspace is needed, so every pointer is judged
    need = _plan(pkg, d)[2]
    assert need == 4 * 4 * 64 * 1 * 4 * 66
    for pos, a in enumerate(ALIGNS):
        b, c = [OK] * 8, [at(1)] * 8                                 # NULL is judged before alignment
        b[pos] = c[pos] = NULL
        assert _call(lib, d, c) == (L.NNOP_ERR_ALIGN if pos in OPTIONAL[:2] else L.NNOP_ERR_NULL), pos
        if pos not in OPTIONAL[:2]:
            assert _call(lib, d, b) == L.NNOP_ERR_NULL, pos
        c = [OK] * 8
        c[pos] = at(a // 2)                                          # aligned to half of what is needed
        assert _call(lib, d, c) == L.NNOP_ERR_ALIGN, pos
    assert _call(lib, d, [OK] * 8, need - 1) == L.NNOP_ERR_WORKSPACE
    one = _desc(pkg, splits=1)                                       # one split: a NULL workspace of 0 bytes passes on to the alignment check
    assert _call(lib, one, [at(1)] * 7 + [NULL], 0) == L.NNOP_ERR_ALIGN and _call(lib, one, [NULL] * 8, 0) == L.NNOP_ERR_NULL


def test_the_plan_follows_the_headers_rule(pkg):
    splits = lambda **kw: _plan(pkg, _desc(pkg, **kw))
    assert splits(batch=1, capacity=65536) == (0, 64, 4 * 64 * 64 * 66)          # ceil(512 / 8) = 64 chunks of 32 tiles
    assert splits(batch=8, capacity=8192) == (0, 8, 4 * 8 * 64 * 8 * 66)
    assert splits(batch=64) == splits(batch=64, capacity=65536) == (0, 1, 0)      # 512 workgroups without a split: no workspace
    assert splits(batch=1, capacity=300) == (0, 2, 4 * 64 * 2 * 66)              # 10 tiles: no chunk below 4
    assert splits(batch=1, capacity=65536, window_left=128) == (0, 1, 0)          # 6 live tiles
    assert splits(batch=1, capacity=100, splits=7) == (0, 7, 4 * 64 * 7 * 66)    # forced: as given
    assert splits(batch=1, emb=128, splits=2, k_stride_l=128, v_stride_l=128)[2] == 4 * 64 * 2 * 130
    for prev, cur in zip((1, 2, 8, 64), (2, 8, 64, 512)):                         # monotone: fewer splits for more sequences or heads,
        assert splits(batch=cur)[1] <= splits(batch=prev)[1]                      # no fewer for a longer cache or a wider window
        assert splits(batch=1, capacity=64 * cur)[1] >= splits(batch=1, capacity=64 * prev)[1]
        assert splits(batch=1, window_left=64 * cur)[1] >= splits(batch=1, window_left=64 * prev)[1]


class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    mk = lambda *s, dt=torch.bfloat16: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    q, k, v, lens = mk(2, 16, 1, 64), mk(2, 2, 40, 64), mk(2, 2, 40, 64), mk(2, dt=torch.int32)
    A, E = pkg.decode_attention, pkg.NNopError
    with pytest.raises(E, match="GPU-only"):
        A(torch.ones(2, 16, 1, 64, dtype=torch.bfloat16), k, v, lens)
    with pytest.raises(E, match="flash_attention"):                              # no autograd, and it names the operator that has one
        A(mk(2, 16, 1, 64, dt=torch.float32).requires_grad_(True).to(torch.bfloat16).as_subclass(OnGpu), k, v, lens)
    for bad, status in ((lambda: A(mk(2, 16, 1, 64, dt=torch.float32), k, v, lens), "NNOP_ERR_DTYPE"),
                        (lambda: A(q, k.to(torch.float16).as_subclass(OnGpu), v, lens), "NNOP_ERR_DTYPE"),
                        (lambda: A(mk(2, 16, 1, 32), mk(2, 2, 40, 32), mk(2, 2, 40, 32), lens), "NNOP_ERR_SHAPE"),
                        (lambda: A(mk(2, 34, 1, 64), k, v, lens), "NNOP_ERR_SHAPE"),              # G = 17
                        (lambda: A(mk(2, 16, 3, 64), k, v, lens), "NNOP_ERR_SHAPE"),              # G QL = 24
                        (lambda: A(q, k, mk(2, 2, 41, 64), lens), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, mk(2, 2, 64, 40).transpose(2, 3), v, lens), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, k, v, mk(3, dt=torch.int32)), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, k, v, mk(2, dt=torch.int64)), "NNOP_ERR_SHAPE"),
                        (lambda: A(q, k, v, lens, sinks=mk(2, dt=torch.float32)), "NNOP_ERR_SHAPE"),
                        (lambda: pkg.decode_attention_into(mk(2, 16, 1, 32), None, q, k, v, lens), "NNOP_ERR_SHAPE")):
        with pytest.raises(E) as e:
            bad()
        assert e.value.status == getattr(pkg._lib, status)
    for bad, exc in ((lambda: A(q, k, v, lens, window_left=-1), ValueError), (lambda: A(q, k, v, lens, window_left=1.5), TypeError),
                     (lambda: A(q, k, v, lens, num_splits=0), ValueError), (lambda: A(q, k, v, lens, num_splits=65), ValueError),
                     (lambda: A(q, k, v, lens, num_splits=True), TypeError), (lambda: A(q, [1], v, lens), TypeError)):
        with pytest.raises(exc):
            bad()
    # both cache layouts become strides, never a copy; the plan needs no device
    d = pkg.decode_attn._desc(q, mk(2, 40, 2, 64).transpose(1, 2), v, 128, 3)
    assert (d.k_stride_b, d.k_stride_h, d.k_stride_l, d.v_stride_b, d.v_stride_h, d.v_stride_l) == (5120, 64, 128, 5120, 2560, 64)
    assert (d.window_left, d.splits, d.capacity, d.qh, d.kh) == (40, 3, 40, 16, 2)     # a window beyond the cache: the capacity, no key fewer
    assert pkg.decode_attn._desc(q, k, v, 2 ** 40, None).window_left == 40 and pkg.decode_attn._desc(q, k, v, 39, None).window_left == 39
    assert pkg.decode_attention_plan(q, k, v, num_splits=3) == (3, 4 * 2 * 16 * 3 * 66) and pkg.decode_attention_plan(q, k, v) == (1, 0)
