"""CPU tests of the decode expert forward with the gated activation in its epilogue (include/nnop_hip_moe_mx_decode_glu.h), the checks
tests/test_zzzzzzzzzz_moe_mx_decode_host.py makes of the eighth library made of the ninth: it loads and exports exactly its header's two
functions, none of the other eight libraries exports them, it links none of them, its header is plain C99 and its descriptor matches the
ctypes one, the binding passes what tests/test_zzzzzz_bindings_host.py asks of the others, the entry point validates in the header's order
and returns before any launch, and the Python wrappers raise before any device work.  Then the gate of tests/moe_mx_glu_ref.py is held
on the CPU: the fp32 evaluation of the formula passes it at every shape and activation of the GPU grid, wrong forms fail it.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import glu_ref
import moe_linear_ref as lin
import moe_mx_glu_ref as ref
import mx_ref
from abi_util import ROOT, strip_c_comments

HEADER = os.path.join(ROOT, "include", "nnop_hip_moe_mx_decode_glu.h")
NAMES = {"nnop_moe_mx_decode_glu_abi_version", "nnop_moe_mx_decode_glu"}
PY_NAMES = ("moe_decode_glu_mxfp4", "_moe_decode_glu_mxfp4", "moe_decode_glu_mxfp4_into")
FIELDS = ["dtype", "rows", "experts", "in_dim", "inter_dim", "ld_x", "ld_h", "ld_b", "ld_q", "ld_s", "act", "layout", "tokens", "topk",
          "alpha", "limit", "flags", "reserved"]
REBUILD = "rebuild with `make -C nnop.jl_amd/csrc -j8`"
ALIGNS, OPTIONAL = ("t", "t", 16, 1, "t", 4, 4), (4, 6)   # h x blocks scales bias offsets perm: the alignment of each ("t" = dtype)
OK = C.c_void_p(0x7f0000001000)                           # never dereferenced: every call in this file returns before a launch
NULL = C.c_void_p(0)
at = lambda off: C.c_void_p(0x7f0000001000 + off)
INF, NAN = float("inf"), float("nan")


# ---- the library, its header, its binding ---------------------------------------------------------------------------------------------
def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_library_exports_exactly_the_headers_functions(pkg):
    M = pkg._lib_moe_mx_decode_glu
    lib = M.load()
    assert set(M.EXPORTED_SYMBOLS) == NAMES
    assert _defined(M.LIB_PATH) == NAMES
    header = strip_c_comments(open(HEADER).read())
    assert set(re.findall(r"\b(nnop_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert lib.nnop_moe_mx_decode_glu_abi_version() == M.MOE_MX_DECODE_GLU_ABI_VERSION == 1
    assert int(re.search(r"#define NNOP_HIP_MOE_MX_DECODE_GLU_ABI_VERSION (\d+)", header).group(1)) == 1
    needed = subprocess.run(["readelf", "-d", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnnop_hip" not in needed                               # none of the other eight libraries
    for name in PY_NAMES:
        assert name in pkg.__all__ and callable(getattr(pkg, name)) and name in pkg.moe_mx_decode_glu.__all__
    assert "moe_mx_decode_glu" in pkg.__all__ and "_lib_moe_mx_decode_glu" in pkg.__all__
    others = (pkg._lib, pkg._lib_ext, pkg._lib_moe, pkg._lib_moe_data, pkg._lib_moe_gemm, pkg._lib_moe_linear, pkg._lib_moe_mx,
              pkg._lib_moe_mx_decode)
    assert len({o.LIB_PATH for o in others} | {M.LIB_PATH}) == 9
    for other in others:
        assert not NAMES & set(other.EXPORTED_SYMBOLS) and not NAMES & _defined(other.LIB_PATH)
    # the eighth library keeps its two symbols
    assert _defined(pkg._lib_moe_mx_decode.LIB_PATH) == {"nnop_moe_mx_decode_abi_version", "nnop_moe_mx_decode_linear"}


def test_descriptor_matches_the_header(pkg):
    M = pkg._lib_moe_mx_decode_glu
    header = strip_c_comments(open(HEADER).read())
    body = re.search(r"typedef struct nnop_moe_mx_decode_glu_desc \{(.*?)\} nnop_moe_mx_decode_glu_desc;", header, re.S).group(1)
    ctypes_of = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    fields = []
    for ctype, names in re.findall(r"(u?int(?:32|64)_t|float)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            fields.append((m.group(1), int(m.group(2) or 1), ctypes_of[ctype]))
    D = M.MoeMxDecodeGluDesc
    assert C.sizeof(D) == 80 and C.sizeof(D) % 8 == 0
    assert [f[0] for f in fields] == FIELDS == [n for n, _ in D._fields_]
    assert [f[1] for f in fields] == [getattr(t, "_length_", 1) for _, t in D._fields_]
    assert [f[2] for f in fields] == [(t._type_ if hasattr(t, "_length_") else t) for _, t in D._fields_]
    assert all(getattr(D, n).size == 4 for n in FIELDS[:-1]) and D.flags.offset == 64 and D.reserved.offset == 68
    assert (M.MAX_EXPERTS, M.MAX_IN, M.MAX_INTER, M.MAX_TOPK, M.BLOCK) == (1024, 65536, 32768, 64, 32)
    # the shared fields lie where the eighth library's descriptor has them
    S = pkg._lib_moe_mx_decode.MoeMxDecodeDesc
    for mine, theirs in (("dtype", "dtype"), ("rows", "rows"), ("experts", "experts"), ("in_dim", "in_dim"), ("inter_dim", "out_dim"),
                         ("ld_x", "ld_x"), ("ld_h", "ld_y"), ("ld_b", "ld_b"), ("ld_q", "ld_q"), ("ld_s", "ld_s")):
        assert getattr(D, mine).offset == getattr(S, theirs).offset
    # the layout values of the header and the activation values of nnop_hip.h
    assert int(re.search(r"#define NNOP_MOE_GLU_INTERLEAVED (\d+)", header).group(1)) == M.LAYOUTS["interleaved"] == 0
    assert int(re.search(r"#define NNOP_MOE_GLU_HALVES\s+(\d+)", header).group(1)) == M.LAYOUTS["halves"] == 1
    assert [pkg._lib.GLU_ACTS[a] for a in glu_ref.ACTS] == [0, 1, 2, 3]


def test_header_compiles_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "nnop_hip_moe_mx_decode_glu.h"\n'
                 "int main(void){ nnop_moe_mx_decode_glu_desc a; a.flags = 0u; a.layout = NNOP_MOE_GLU_HALVES;\n"
                 "  return (sizeof(a) == 80 && NNOP_HIP_MOE_MX_DECODE_GLU_ABI_VERSION == 1 && a.flags == 0u && a.layout == 1) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")],
                   check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_the_bindings_glue_holds_for_the_ninth_library(pkg, monkeypatch):
    """the three checks tests/test_zzzzzz_bindings_host.py makes of the other bindings, and its check of an operator module"""
    M, common, module = pkg._lib_moe_mx_decode_glu, pkg._common, pkg.moe_mx_decode_glu
    lib = M.load()
    assert M.load() is lib is M._lib and M.EXPORTED_SYMBOLS == tuple(M.PROTOTYPES)
    for name, (restype, argtypes) in M.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
    assert module.NNopError is common.NNopError and module._DTYPES is common._DTYPES
    for name in ("_ptr", "_stream", "_on_device", "_raise", "_launch", "_dtype_name"):
        assert vars(module).get(name, getattr(common, name)) is getattr(common, name), name
    assert "_ptr" in vars(module)
    # the checks, the recomputation and the pullbacks are the other modules' own, not copies
    assert module._check is pkg.moe_mx._check and module._offsets is pkg.moe_gemm._offsets and module._bias is pkg.moe_linear._bias
    assert module._rows is pkg.moe._rows and module._out_rows is pkg.moe_data._out_rows
    assert module._moe_decode_linear_mxfp4 is pkg.moe_mx_decode._moe_decode_linear_mxfp4
    assert module.grad_glu_packed is pkg.activations.grad_glu_packed and module._act is pkg.activations._act
    assert module.grad_moe_grouped_linear_mxfp4_x_into is pkg.moe_mx.grad_moe_grouped_linear_mxfp4_x_into
    assert module.grad_moe_grouped_linear_b_into is pkg.moe_linear.grad_moe_grouped_linear_b_into
    assert (module.OAI_ALPHA, module.OAI_LIMIT) == (pkg.activations.OAI_ALPHA, pkg.activations.OAI_LIMIT) == (1.702, 7.0)
    monkeypatch.setattr(M, "_lib", None)
    monkeypatch.setattr(M, "MOE_MX_DECODE_GLU_ABI_VERSION", 2)
    with pytest.raises(pkg._lib.NNopLibraryMissing) as e:
        M.load()
    assert str(e.value) == f"{M.LIB_PATH} has moe-mx-decode-glu-ABI version 1, this binding needs 2: {REBUILD}"
    monkeypatch.setattr(M, "MOE_MX_DECODE_GLU_ABI_VERSION", 1)
    monkeypatch.setattr(M, "EXPORTED_SYMBOLS", M.EXPORTED_SYMBOLS + ("nnop_not_there",))
    with pytest.raises(pkg._lib.NNopLibraryMissing) as e:
        M.load()
    assert str(e.value) == f"{M.LIB_PATH} does not export nnop_not_there: {REBUILD}"
    monkeypatch.setattr(M, "LIB_PATH", "/nonexistent/libnnop.so")
    with pytest.raises(pkg._lib.NNopLibraryMissing) as e:
        M.load()
    assert str(e.value) == ("/nonexistent/libnnop.so not found: build it with `make -C nnop.jl_amd/csrc -j8` "
                            "(or __graft_entry__.build()).  There is no CPU or PyTorch fallback.")
    assert M._lib is None                        # a refused load leaves nothing behind


# ---- validation: order and codes, before any launch -----------------------------------------------------------------------------------
def _desc(pkg, reserved=(0, 0, 0), **kw):
    base = dict(dtype=2, rows=256, experts=8, in_dim=128, inter_dim=32, ld_x=128, ld_h=32, ld_b=64, ld_q=64, ld_s=4, act=3, layout=0,
                tokens=0, topk=0, alpha=1.702, limit=7.0, flags=0)
    base.update(kw)
    d = pkg._lib_moe_mx_decode_glu.MoeMxDecodeGluDesc(**base)
    for i, r in enumerate(reserved):
        d.reserved[i] = r
    return d


def _call(lib, d, ptrs):
    return lib.nnop_moe_mx_decode_glu(C.byref(d) if d is not None else None, *ptrs, None)


def _all(lib, d, ptr=OK, perm=None):
    """every pointer `ptr`; perm follows the descriptor (given exactly when tokens is not 0) unless it is named"""
    p = [ptr] * len(ALIGNS)
    p[6] = ((ptr if d is not None and d.tokens != 0 else NULL) if perm is None else perm)
    return _call(lib, d, p)


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=0), "NNOP_ERR_DTYPE"),                               # fp32 rows beside packed weights
    (dict(dtype=9), "NNOP_ERR_DTYPE"),
    (dict(dtype=-1), "NNOP_ERR_DTYPE"),
    (dict(flags=1), "NNOP_ERR_OPTS"),
    (dict(flags=0x80000000), "NNOP_ERR_OPTS"),
    (dict(reserved=(1, 0, 0)), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, -1, 0)), "NNOP_ERR_OPTS"),
    (dict(reserved=(0, 0, 7)), "NNOP_ERR_OPTS"),
    (dict(act=-1), "NNOP_ERR_OPTS"),                                 # nnop_glu's option checks
    (dict(act=4), "NNOP_ERR_OPTS"),
    (dict(layout=2), "NNOP_ERR_OPTS"),
    (dict(layout=-1), "NNOP_ERR_OPTS"),
    (dict(alpha=INF), "NNOP_ERR_OPTS"),
    (dict(alpha=NAN), "NNOP_ERR_OPTS"),
    (dict(limit=0.0), "NNOP_ERR_OPTS"),
    (dict(limit=-7.0), "NNOP_ERR_OPTS"),
    (dict(limit=INF), "NNOP_ERR_OPTS"),
    (dict(limit=NAN), "NNOP_ERR_OPTS"),
    (dict(rows=0), "NNOP_ERR_SHAPE"),
    (dict(rows=-3), "NNOP_ERR_SHAPE"),
    (dict(experts=0), "NNOP_ERR_SHAPE"),
    (dict(experts=1025), "NNOP_ERR_SHAPE"),
    (dict(in_dim=0), "NNOP_ERR_SHAPE"),
    (dict(inter_dim=0), "NNOP_ERR_SHAPE"),
    (dict(in_dim=65568, ld_x=65568, ld_q=32784, ld_s=2049), "NNOP_ERR_SHAPE"),
    (dict(inter_dim=32769, ld_h=32769, ld_b=65538), "NNOP_ERR_SHAPE"),           # N = 2 I above 65536
    (dict(in_dim=120, ld_x=120), "NNOP_ERR_SHAPE"),                  # K no multiple of 32
    (dict(in_dim=16, ld_x=16), "NNOP_ERR_SHAPE"),
    (dict(ld_x=127), "NNOP_ERR_SHAPE"),                              # ld = dim - 1, each stride
    (dict(ld_h=31), "NNOP_ERR_SHAPE"),
    (dict(ld_b=63), "NNOP_ERR_SHAPE"),                               # the bias row has 2 I columns
    (dict(ld_q=48), "NNOP_ERR_SHAPE"),                               # below K / 2
    (dict(ld_q=72), "NNOP_ERR_SHAPE"),                               # no multiple of 16
    (dict(ld_s=3), "NNOP_ERR_SHAPE"),
    (dict(tokens=-1, topk=4), "NNOP_ERR_SHAPE"),
    (dict(tokens=64, topk=-4), "NNOP_ERR_SHAPE"),
    (dict(tokens=64, topk=0), "NNOP_ERR_SHAPE"),                     # one of the two alone
    (dict(tokens=0, topk=4), "NNOP_ERR_SHAPE"),
    (dict(tokens=64, topk=65), "NNOP_ERR_SHAPE"),
    (dict(tokens=2 ** 31 - 1, topk=2), "NNOP_ERR_SHAPE"),            # T k above 2^31 - 1
    (dict(tokens=2 ** 26, topk=32), "NNOP_ERR_SHAPE"),
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=0, flags=8, rows=0), "NNOP_ERR_DTYPE"),
    (dict(dtype=7, act=9, in_dim=120), "NNOP_ERR_DTYPE"),
    (dict(reserved=(0, 3, 0), rows=0), "NNOP_ERR_OPTS"),
    (dict(flags=16, ld_q=72), "NNOP_ERR_OPTS"),
    (dict(act=7, rows=0), "NNOP_ERR_OPTS"),
    (dict(layout=5, tokens=-1), "NNOP_ERR_OPTS"),
    (dict(limit=-1.0, inter_dim=0), "NNOP_ERR_OPTS"),
])
def test_descriptor_validation(pkg, kw, status):
    lib, want = pkg._lib_moe_mx_decode_glu.load(), getattr(pkg._lib, status)
    d = _desc(pkg, **kw)
    assert _all(lib, d) == want
    assert _all(lib, d, NULL) == want                                # the descriptor is judged before the pointers
    assert _all(lib, d, at(1)) == want


def test_alpha_and_limit_are_judged_for_swiglu_oai_only(pkg):
    lib, L = pkg._lib_moe_mx_decode_glu.load(), pkg._lib
    for act in (0, 1, 2):
        for kw in (dict(alpha=NAN), dict(limit=-1.0), dict(limit=NAN), dict(alpha=INF, limit=0.0)):
            assert _all(lib, _desc(pkg, act=act, **kw), NULL) == L.NNOP_ERR_NULL, (act, kw)


def test_perm_and_the_token_fields_go_together(pkg):
    """a perm that is NULL while tokens / topk are not 0, or the reverse, is NNOP_ERR_SHAPE, judged with the descriptor"""
    lib, L = pkg._lib_moe_mx_decode_glu.load(), pkg._lib
    with_perm, without = _desc(pkg, tokens=64, topk=4), _desc(pkg)
    for ptr in (OK, NULL, at(1)):
        assert _all(lib, with_perm, ptr, perm=NULL) == L.NNOP_ERR_SHAPE
        assert _all(lib, without, ptr, perm=OK) == L.NNOP_ERR_SHAPE
    assert _all(lib, with_perm, NULL, perm=OK) == L.NNOP_ERR_NULL    # consistent: on to the pointers
    assert _all(lib, without, NULL) == L.NNOP_ERR_NULL
    for ok in (dict(tokens=1, topk=1), dict(tokens=64, topk=64), dict(tokens=2 ** 31 - 1, topk=1), dict(tokens=2 ** 25, topk=63)):
        assert _all(lib, _desc(pkg, **ok), NULL, perm=OK) == L.NNOP_ERR_NULL, ok


def test_valid_descriptors_reach_the_pointer_checks(pkg):
    """the largest shapes included: E ceil(I / 128) workgroups stay below 2^31 for every E and I the bounds admit, whatever S is"""
    lib, L = pkg._lib_moe_mx_decode_glu.load(), pkg._lib
    for ok in (dict(), dict(dtype=1), dict(layout=1), dict(act=0), dict(act=1, layout=1), dict(act=2),
               dict(rows=1, experts=1, in_dim=32, inter_dim=1, ld_x=32, ld_h=1, ld_b=2, ld_q=16, ld_s=1),
               dict(experts=1024), dict(ld_q=80, ld_s=9, ld_x=131, ld_h=35, ld_b=70), dict(inter_dim=5, ld_h=5, ld_b=10),
               dict(in_dim=65536, ld_x=65536, ld_q=32768, ld_s=2048), dict(inter_dim=32768, ld_h=32768, ld_b=65536),
               dict(rows=2 ** 31 - 1, in_dim=32, inter_dim=8, ld_x=32, ld_h=8, ld_b=16, ld_q=16, ld_s=1),
               dict(rows=2 ** 31 - 1, experts=1024, in_dim=65536, inter_dim=32768, ld_x=65536, ld_h=32768, ld_b=65536, ld_q=32768, ld_s=2048)):
        assert _all(lib, _desc(pkg, **ok), NULL) == L.NNOP_ERR_NULL, ok
    assert _all(lib, None) == L.NNOP_ERR_NULL                        # the descriptor itself: first of all
    assert _all(lib, None, at(1)) == L.NNOP_ERR_NULL


def test_null_and_alignment_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib_moe_mx_decode_glu.load(), pkg._lib
    n = len(ALIGNS)
    for dtype in (1, 2):
        d = _desc(pkg, dtype=dtype, tokens=64, topk=4)               # with perm, so that every pointer is judged
        for pos, a in enumerate(ALIGNS):
            if pos == 6:
                continue                                             # perm NULL beside tokens: the descriptor's check, above
            b, c = [OK] * n, [at(1)] * n                             # NULL is judged before alignment
            b[pos] = c[pos] = NULL
            if pos in OPTIONAL:                                      # bias: NULL means none, so the call goes on to the next check
                assert _call(lib, d, c) == L.NNOP_ERR_ALIGN, pos
            else:
                assert _call(lib, d, b) == L.NNOP_ERR_NULL, pos
                assert _call(lib, d, c) == L.NNOP_ERR_NULL, pos
        for pos, a in enumerate(ALIGNS):
            size = 2 if a == "t" else a
            if size > 1:                                             # scales: bytes, any address
                c = [OK] * n
                c[pos] = at(size // 2)                               # aligned to half of what is needed
                assert _call(lib, d, c) == L.NNOP_ERR_ALIGN, (pos, a)


# ---- the Python wrappers ---------------------------------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):
    """a CPU tensor that claims to be on the GPU reaches the host checks, which run in front of any device work"""
    is_cuda = True


def test_python_checks_raise_before_device_work(pkg):
    S, E, I, K = 12, 3, 6, 64
    N = 2 * I
    f = lambda *s, dt=torch.bfloat16: torch.ones(*s, dtype=dt)
    u = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    x, h, q, sc, b, off = f(S, K), f(S, I), u(E, N, 2, 16), u(E, N, 2), f(E, N), torch.zeros(E + 1, dtype=torch.int32)
    for call in (lambda: pkg.moe_decode_glu_mxfp4(x, q, sc, off), lambda: pkg._moe_decode_glu_mxfp4(x, q, sc, off, b),
                 lambda: pkg.moe_decode_glu_mxfp4_into(h, x, q, sc, off, b),
                 lambda: pkg.moe_decode_glu_mxfp4(x.clone().requires_grad_(True), q, sc, off, b),
                 lambda: pkg.moe_decode_glu_mxfp4(x, q, sc, off, b.clone().requires_grad_(True))):
        with pytest.raises(pkg.NNopError, match="GPU-only"):
            call()
    mk = lambda *s, dt=torch.bfloat16: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    mu = lambda *s: torch.zeros(*s, dtype=torch.uint8).as_subclass(OnGpu)
    mi = lambda *s: torch.zeros(*s, dtype=torch.int32).as_subclass(OnGpu)
    x, h, q, sc, b, off = mk(S, K), mk(S, I), mu(E, N, 2, 16), mu(E, N, 2), mk(E, N), mi(E + 1)
    G = pkg.moe_decode_glu_mxfp4
    for call in (lambda: G(x, q, sc, off, act="relu"), lambda: G(x, q, sc, off, layout="split"), lambda: G(x, q, sc, off, layout=None),
                 lambda: pkg._moe_decode_glu_mxfp4(x, q, sc, off, act="swish"), lambda: pkg.moe_decode_glu_mxfp4_into(h, x, q, sc, off, layout=1)):
        with pytest.raises(ValueError, match="unknown"):
            call()
    for call in (lambda: G(mk(S, K, dt=torch.float64), q, sc, off), lambda: G(x, [1], sc, off), lambda: G(x, q, sc, off, mi(E, N)),
                 lambda: G(x, q, sc, off.long()), lambda: G(mk(3, K), q, sc, off, perm=mi(S).long(), k=4), lambda: G(mk(3, K), q, sc, off, perm=[0] * S, k=4)):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(pkg.NNopError, match="must be float16 or bfloat16") as e:     # fp32 rows beside packed weights
        G(mk(S, K, dt=torch.float32), q, sc, off)
    assert e.value.status == pkg._lib.NNOP_ERR_DTYPE
    with pytest.raises(pkg.NNopError, match="2 I rows") as e:                        # an odd number of weight rows
        G(x, mu(E, 7, 2, 16), mu(E, 7, 2), off)
    assert e.value.status == pkg._lib.NNOP_ERR_SHAPE
    for bad in (lambda: G(x, q.to(torch.int8).as_subclass(OnGpu), sc, off), lambda: G(x, q, mk(E, N, 2), off),
                lambda: G(x, mu(E, N, 16, 2).transpose(2, 3), sc, off), lambda: G(x, mu(E, N, 2, 8), sc, off),
                lambda: G(x, mu(E, N + 2, 2, 16), sc, off), lambda: G(mk(S, K + 32), q, sc, off), lambda: G(mk(S, K, dt=torch.float16), q, sc, off, b),
                lambda: G(x, q, sc, off, mk(E, I)), lambda: G(x, q, sc, off, mk(E, N + 1)), lambda: G(x, q, sc, mi(E)),
                lambda: pkg.moe_decode_glu_mxfp4_into(mk(S, N), x, q, sc, off), lambda: pkg.moe_decode_glu_mxfp4_into(mk(I, S).t(), x, q, sc, off),
                lambda: pkg.moe_decode_glu_mxfp4_into(h, mk(4, K), q, sc, off, perm=mi(16), k=4),     # h must have T k rows ...
                lambda: G(mk(3, K), q, sc, off, perm=mi(S + 1), k=4), lambda: G(mk(3, K), q, sc, off, perm=mi(3, 4), k=4)):  # ... and perm T k entries
        with pytest.raises(pkg.NNopError, match="must"):
            bad()
    for call in (lambda: G(mk(0, K), q, sc, off), lambda: G(x, mu(1025, N, 2, 16), mu(1025, N, 2), mi(1026)),
                 lambda: G(x, q, sc, off, k=4), lambda: G(mk(3, K), q, sc, off, perm=mi(S)), lambda: G(mk(3, K), q, sc, off, perm=mi(S), k=0),
                 lambda: G(mk(3, K), q, sc, off, perm=mi(195), k=65), lambda: G(mk(3, K), q, sc, off, perm=mi(S), k=4.0)):
        with pytest.raises(pkg.NNopError) as e:
            call()
        assert e.value.status == pkg._lib.NNOP_ERR_SHAPE
    # a gradient through perm is refused by name, in front of any device work
    with pytest.raises(pkg.NNopError, match="moe_permute, moe_decode_linear_mxfp4 and glu_packed"):
        G(mk(3, K).requires_grad_(True), q, sc, off, perm=mi(S), k=4)
    # the descriptor a call builds: the packed strides are the dense ones, unused row strides too
    d = pkg.moe_mx_decode_glu._desc(torch.zeros(3, 96, dtype=torch.float16), 3, 4, 96, 12, 3, 1, 1.5, 6.0, ld_x=99, ld_h=16)
    assert [getattr(d, n) for n, _ in d._fields_[:-1]] == [1, 3, 4, 96, 12, 99, 16, 24, 48, 3, 3, 1, 0, 0, 1.5, 6.0, 0] and tuple(d.reserved) == (0,) * 3
    d = pkg.moe_mx_decode_glu._desc(torch.zeros(3, 96, dtype=torch.bfloat16), 12, 4, 96, 12, 0, 0, 1.702, 7.0, 3, 4)
    assert (d.rows, d.tokens, d.topk, d.ld_x, d.ld_h, d.ld_b) == (12, 3, 4, 96, 12, 24)


# ---- the gate, held on the CPU ----------------------------------------------------------------------------------------------------------
KIS = ((32, 4), (64, 12), (96, 68), (544, 132), (160, 5), (2880, 24))       # the shapes of the GPU grid
COUNTS = [1, 15, 16, 17, 31, 33, 63, 64]
_INPUTS = {}


def _inputs(K, I, dt, layout):
    """computed once per (shape, type, layout) and left unchanged: rows, dequantised weights, offsets, bias"""
    key = (K, I, dt, layout)
    if key not in _INPUTS:
        off = lin.offsets_of(COUNTS)
        S, E = int(off[-1]) + 1, len(COUNTS)
        blocks, scales = mx_ref.random_packed(10 * K + I, (E, 2 * I, K))
        w = mx_ref.dequant(blocks, scales, dt)
        x = lin.make(K + I, (S, K), dt)
        x = x * np.float32(ref.x_scale(x, w, off, layout))
        _INPUTS[key] = (x, w, off, lin.make(K + I + 1, (E, 2 * I), dt))
    return _INPUTS[key]


CPU_GRID = [(K, I, "swiglu_oai") for K, I in KIS] + [(K, I, act) for act in glu_ref.ACTS[:3] for K, I in (KIS[2], KIS[3])]


@pytest.mark.parametrize("layout", ref.LAYOUTS)
@pytest.mark.parametrize("dt", ("f16", "bf16"))
@pytest.mark.parametrize("K,I,act", CPU_GRID, ids=[f"K{k}-I{i}-{a}" for k, i, a in CPU_GRID])
def test_the_fp32_formula_passes_the_gate_and_wrong_forms_fail_it(K, I, act, dt, layout):
    """the formula evaluated in fp32 with one rounding, the product in BLAS order and (K <= 544) in one sequential chain, lies inside the
    gate; the last 8 terms dropped, expert e on the weights of expert e + 1, gate and up swapped, and for swiglu_oai a missing + 1 on the up
    side or a missing clamp lie outside.  The form that rounds p to the element type in front of the activation is printed, not judged"""
    x, w, off, bias = _inputs(K, I, dt, layout)
    want = ref.glu_decode_ref(x, w, off, bias, act, layout)
    if want["h"].size >= 1024 and act == "swiglu_oai":
        assert min(ref.saturation(want, inside=lin.rows_of(off, x.shape[0]) >= 0)) >= 0.02
    ratio = lambda **kw: ref.worst(ref.glu_decode_f32(x, w, off, dt, bias, act, layout, **kw), want, dt)
    good = {"blas": ratio()}
    if K <= 544:
        good["chain"] = ratio(order="seq")
    print(f"K{K} I{I} {act} {layout} [{dt}] fp32 forms / gate: {good}  rounded p / gate: {ratio(round_p=True):.3f}")
    assert all(0 < r <= 1.0 for r in good.values()), good
    wrong = dict(short=ratio(short=8), shift=ratio(shift=1), swap=ratio(swap=True))
    if act == "swiglu_oai":
        wrong.update(no_plus_one=ratio(plus1=False), no_clamp=ratio(clamp=False))
    assert all(r > 1.0 for r in wrong.values()), wrong
    # no bias, and rows outside every expert: +0 in the reference, and the gate there is the floor alone
    none = ref.glu_decode_ref(x, w, off, None, act, layout)
    assert ref.worst(ref.glu_decode_f32(x, w, off, dt, None, act, layout), none, dt) <= 1.0
    assert not none["h"][-1].any() and not want["h"][-1].any()


def test_the_reference_helpers():
    """split / to_halves are inverse views of one projection, gather is moe_permute's formula, L bounds |a'| of the four activations"""
    p = np.arange(24.0).reshape(2, 12)
    g0, u0 = ref.split(p, "interleaved")
    g1, u1 = ref.split(ref.to_halves(p, 1), "halves")
    assert (g0 == g1).all() and (u0 == u1).all() and (g0[0] == [0, 2, 4, 6, 8, 10]).all()
    x = np.arange(12.0).reshape(4, 3)
    xs = ref.gather(x, np.array([7, -1, 0, 8, 3, 2 ** 31 - 1]), 2)
    assert (xs == np.stack([x[3], 0 * x[0], x[0], 0 * x[0], x[1], 0 * x[0]])).all()
    grid = torch.linspace(-12, 12, 48001, dtype=torch.float64)
    for act in glu_ref.ACTS:
        for alpha in (0.5, 1.0, 1.702, 4.0):
            assert float(glu_ref.act_ref(grid, act, alpha, 100.0)[1].abs().max()) <= ref.L_ACT
