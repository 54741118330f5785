"""CPU tests of the gated MLP activations (include/nnop_hip.h, nnop_glu / nnop_glu_bwd): the two entry points are declared, bound and
exported; they validate descriptor, pointers and alignment in that order and return before any launch; the Python wrappers refuse CPU
tensors, a mismatched `up` and unknown names before any device work; the reference the GPU tests are judged against (tests/glu_ref.py)
has the right gradient; and the GPU tests' tolerance is restated as a model that computes in fp32 and rounds once.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import ctypes as C
import math
import re

import pytest
import torch

import glu_ref as ref
from abi_util import HEADER, SHIM, strip_c_comments

NEW = ("nnop_glu", "nnop_glu_bwd")
OK = C.c_void_p(0x7f0000001000)              # never dereferenced: every call in this file returns before a launch
NULL = C.c_void_p(0)


def test_exports(pkg):
    header = strip_c_comments(open(HEADER).read())
    declared = set(re.findall(r"\b(nnop_[a-z_]+)\s*\(", header))
    lib = pkg._lib.load()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/nnop_hip.h"
        assert name in pkg._lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert getattr(lib, name).argtypes is not None
    assert len(lib.nnop_glu.argtypes) == 5 and len(lib.nnop_glu_bwd.argtypes) == 7
    assert lib.nnop_abi_version() == 7 and pkg._lib.ABI_VERSION == 7
    assert C.sizeof(pkg._lib.GluDesc) == 48
    for e in ("NNOP_GLU_SILU", "NNOP_GLU_GELU_TANH", "NNOP_GLU_GELU_ERF", "NNOP_GLU_SWIGLU_OAI", "NNOP_GLU_SPLIT", "NNOP_GLU_INTERLEAVED"):
        assert re.search(r"\b%s\s*=\s*\d" % e, header), e
    assert pkg._lib.GLU_ACTS == {"silu": 0, "gelu_tanh": 1, "gelu_erf": 2, "swiglu_oai": 3}


def _desc(pkg, **kw):
    base = dict(dtype=2, act=0, layout=0, reserved=0, rows=64, n=1024, ld=1024, alpha=1.702, limit=7.0)
    base.update(kw)
    return pkg._lib.GluDesc(**base)


def _both(lib, d, il=False, p=OK):
    """(nnop_glu, nnop_glu_bwd) with every required pointer = p and up / dup absent exactly when the layout is interleaved"""
    up = NULL if il else p
    return [lib.nnop_glu(C.byref(d), p, p, up, None), lib.nnop_glu_bwd(C.byref(d), p, up, p, p, up, None)]


INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=9), "NNOP_ERR_DTYPE"),
    (dict(dtype=-1), "NNOP_ERR_DTYPE"),
    (dict(act=4), "NNOP_ERR_OPTS"),
    (dict(act=-1), "NNOP_ERR_OPTS"),
    (dict(layout=2), "NNOP_ERR_OPTS"),
    (dict(act=3, alpha=INF), "NNOP_ERR_OPTS"),
    (dict(act=3, alpha=NAN), "NNOP_ERR_OPTS"),
    (dict(act=3, limit=0.0), "NNOP_ERR_OPTS"),
    (dict(act=3, limit=-7.0), "NNOP_ERR_OPTS"),
    (dict(act=3, limit=INF), "NNOP_ERR_OPTS"),
    (dict(act=3, limit=NAN), "NNOP_ERR_OPTS"),
    (dict(rows=0), "NNOP_ERR_SHAPE"),
    (dict(rows=-3), "NNOP_ERR_SHAPE"),
    (dict(n=0), "NNOP_ERR_SHAPE"),
    (dict(reserved=1), "NNOP_ERR_SHAPE"),
    (dict(ld=1023), "NNOP_ERR_SHAPE"),                       # split: ld < n
    (dict(layout=1, ld=1024), "NNOP_ERR_SHAPE"),             # interleaved: ld must be 2n
    (dict(layout=1, ld=2056), "NNOP_ERR_SHAPE"),
    # the order: dtype before options before shape, all before the pointers
    (dict(dtype=9, act=7, rows=0), "NNOP_ERR_DTYPE"),
    (dict(act=7, rows=0), "NNOP_ERR_OPTS"),
    (dict(act=3, limit=NAN, n=0), "NNOP_ERR_OPTS"),
])
def test_descriptor_validation(pkg, kw, status):
    d = _desc(pkg, **kw)
    want = getattr(pkg._lib, status)
    lib = pkg._lib.load()
    il = kw.get("layout") == 1
    assert _both(lib, d, il) == [want] * 2
    # the descriptor is judged before the pointers: all NULL changes nothing
    assert [lib.nnop_glu(C.byref(d), NULL, NULL, NULL, None), lib.nnop_glu_bwd(C.byref(d), NULL, NULL, NULL, NULL, NULL, None)] == [want] * 2


@pytest.mark.parametrize("kw", [
    dict(rows=2 ** 36, n=1024, ld=1024),                     # 2^35 workgroups
    dict(rows=2 ** 36, n=1024, ld=2048, layout=1),
    dict(rows=2 ** 33, n=1023, ld=1023),                     # element-wise path: 2^35 workgroups again
    dict(rows=2 ** 62, n=2 ** 40, ld=2 ** 40),               # rows * ld does not fit 64 bits
    dict(rows=2 ** 20, n=1, ld=2 ** 62),
])
def test_a_grid_that_does_not_fit_is_a_shape_error(pkg, kw):
    """valid descriptor, valid (fake, aligned) pointers, more work than one launch takes: NNOP_ERR_SHAPE, and nothing is launched"""
    lib = pkg._lib.load()
    for dtype in (0, 2):
        d = _desc(pkg, dtype=dtype, **kw)
        assert _both(lib, d, kw.get("layout") == 1) == [pkg._lib.NNOP_ERR_SHAPE] * 2


def test_alpha_and_limit_are_ignored_unless_oai(pkg):
    lib = pkg._lib.load()
    for act in (0, 1, 2):
        d = _desc(pkg, act=act, alpha=NAN, limit=-1.0)
        assert _both(lib, d, p=NULL) == [pkg._lib.NNOP_ERR_NULL] * 2          # the descriptor passed
    assert lib.nnop_glu(None, OK, OK, OK, None) == pkg._lib.NNOP_ERR_NULL


def test_null_and_alignment_checks_come_before_any_launch(pkg):
    lib, L = pkg._lib.load(), pkg._lib
    odd = C.c_void_p(0x7f0000001001)
    two = C.c_void_p(0x7f0000001002)
    for layout in (0, 1):
        d = _desc(pkg, layout=layout, ld=2048 if layout else 1024)
        up = NULL if layout else OK
        fwd, bwd = [OK, OK, up], [OK, up, OK, OK, up]
        for args, fn in ((fwd, lib.nnop_glu), (bwd, lib.nnop_glu_bwd)):
            for pos, a in enumerate(args):
                b = list(args)
                if a is NULL:                                # up / dup given with the interleaved layout
                    b[pos] = OK
                else:
                    b[pos] = NULL
                assert fn(C.byref(d), *b, None) == L.NNOP_ERR_NULL, (layout, fn.__name__, pos)
                if a is not NULL:
                    # NULL is judged before alignment: one NULL and one misaligned pointer is NNOP_ERR_NULL ...
                    c = [odd if x is not NULL else x for x in args]
                    c[pos] = NULL
                    assert fn(C.byref(d), *c, None) == L.NNOP_ERR_NULL
                    # ... and a base that is not a multiple of the element size is NNOP_ERR_ALIGN
                    c = list(args)
                    c[pos] = odd
                    assert fn(C.byref(d), *c, None) == L.NNOP_ERR_ALIGN, (layout, fn.__name__, pos)
    # fp32: 2-byte alignment is not enough
    d = _desc(pkg, dtype=0)
    assert lib.nnop_glu(C.byref(d), two, OK, OK, None) == L.NNOP_ERR_ALIGN
    assert lib.nnop_glu_bwd(C.byref(d), OK, OK, OK, OK, two, None) == L.NNOP_ERR_ALIGN
    for st in (L.NNOP_ERR_OPTS, L.NNOP_ERR_ALIGN):
        assert "glu" in L.strerror(st)


def test_python_checks(pkg):
    g = torch.ones(4, 32)
    for call in (lambda: pkg.glu(g, g), lambda: pkg.swiglu(g, g), lambda: pkg.geglu(g, g), lambda: pkg._glu(g, g),
                 lambda: pkg.glu_packed(g), lambda: pkg.glu_packed(g, act="swiglu_oai"), lambda: pkg.grad_glu(g, g, g),
                 lambda: pkg.grad_glu_packed(torch.ones(4, 16), g), lambda: pkg.glu_into(g.clone(), g, g),
                 lambda: pkg.grad_glu_into(g.clone(), g.clone(), g, g, g),
                 lambda: pkg.glu(g.clone().requires_grad_(True), g), lambda: pkg.glu_packed(g.clone().requires_grad_(True))):
        with pytest.raises(pkg.NNopError, match="GPU-only"):
            call()
    assert pkg.workmodel.glu_bytes(14336, 8192, 2) == 3 * 14336 * 8192 * 2
    assert pkg.workmodel.glu_bytes(14336, 8192, 2, bwd=True) == 5 * 14336 * 8192 * 2
    assert pkg.workmodel.glu_bytes(1024, 1024, 4) == 12 * 2 ** 20 and pkg.workmodel.glu_bytes(1, 1, 4, bwd=True) == 20


def test_mismatches_and_unknown_names_raise_before_device_work(pkg):
    """CPU tensors that claim to be on the GPU reach the host checks, which run in front of any device work"""
    class OnGpu(torch.Tensor):
        is_cuda = True

    mk = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    g = mk(4, 32)
    for bad in (mk(4, 31), mk(5, 32), mk(4, 32, dt=torch.float16), mk(32)):
        for call in (lambda: pkg._glu(g, bad), lambda: pkg.glu(g, bad), lambda: pkg.glu(g.clone().requires_grad_(True), bad),
                     lambda: pkg.grad_glu(g, g, bad), lambda: pkg.glu_into(mk(4, 32), g, bad),
                     lambda: pkg.grad_glu_into(mk(4, 32), mk(4, 32), g, g, bad)):
            with pytest.raises(TypeError, match="up"):
                call()
    with pytest.raises(TypeError, match="dy"):
        pkg.grad_glu(mk(4, 31), g, g)
    with pytest.raises(TypeError, match="dy"):
        pkg.grad_glu_packed(mk(4, 32), g)                    # dy of a packed [4, 32] is [4, 16]
    with pytest.raises(TypeError, match="2n"):
        pkg.glu_packed(mk(4, 31))
    with pytest.raises(TypeError):
        pkg._glu(mk(4, 32, dt=torch.float64), mk(4, 32, dt=torch.float64))
    for call in (lambda: pkg.glu(g, g, act="relu"), lambda: pkg._glu(g, g, act="gelu"), lambda: pkg.grad_glu(g, g, g, act=""),
                 lambda: pkg.glu_packed(g, act="swish"), lambda: pkg.glu_packed(g, layout="rows"),
                 lambda: pkg.grad_glu_packed(mk(4, 16), g, layout="split"), lambda: pkg.geglu(g, g, approximate="erf")):
        with pytest.raises(ValueError):
            call()


def test_row_stride_of_views(pkg):
    """what is handed over by stride: rows of unit stride one common stride apart once the leading dims are flattened"""
    rs = pkg.activations._row_stride
    gu = torch.zeros(2, 17, 96)
    a, b = gu.chunk(2, -1)
    assert rs(gu) == 96 and rs(a) == 96 and rs(b) == 96 and rs(gu[..., :40]) == 96
    assert rs(gu[:, :5]) is None                             # the batch stride is not 5 rows
    assert rs(gu[:, :, ::2]) is None and rs(gu.transpose(0, 1)) is None
    assert rs(gu[:1, :5, 8:16]) == 96 and rs(gu[0, 3]) == 96 and rs(torch.zeros(7)) == 7
    assert rs(torch.zeros(5, 1).expand(5, 8)) is None and rs(torch.zeros(1, 8).expand(5, 8)) is None
    g2, u2, ld = pkg.activations._by_stride(a, b)
    assert g2 is a and u2 is b and ld == 96
    g2, u2, ld = pkg.activations._by_stride(a, torch.zeros(2, 17, 48))
    assert ld == 48 and g2.is_contiguous() and u2.is_contiguous()


# ---- the reference ----------------------------------------------------------------------------------------------------
def _inputs(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    g = 3 * torch.randn(shape, generator=gen, dtype=torch.float64)
    u = 3 * torch.randn(shape, generator=gen, dtype=torch.float64)
    dy = torch.randn(shape, generator=gen, dtype=torch.float64)
    return g, u, dy


@pytest.mark.parametrize("act", ref.ACTS)
def test_reference_gradients_match_finite_differences(act):
    g, u, dy = _inputs((6, 50), 0)
    if act == "swiglu_oai":                                  # keep away from the clamp bounds: the function has a kink there
        for t in (g, u):
            near = ((t.abs() - ref.OAI_LIMIT).abs() < 1e-3)
            t[near] += 0.01
    dg, du = ref.glu_grads_ref(dy, g, u, act)
    h = 1e-6
    fd_g = (ref.glu_ref(g + h, u, act) - ref.glu_ref(g - h, u, act)) / (2 * h) * dy
    fd_u = (ref.glu_ref(g, u + h, act) - ref.glu_ref(g, u - h, act)) / (2 * h) * dy
    assert (fd_g - dg).abs().max() < 1e-7 * max(1.0, float(dg.abs().max()))
    assert (fd_u - du).abs().max() < 1e-7 * max(1.0, float(du.abs().max()))


@pytest.mark.parametrize("act", ref.ACTS)
def test_reference_matches_autograd_of_the_textbook_formulas(act):
    g, u, dy = _inputs((6, 50), 1)
    gd, ud = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
    y = ref.textbook(gd, ud, act)
    y.backward(dy)
    torch.testing.assert_close(ref.glu_ref(g, u, act), y.detach(), rtol=1e-12, atol=1e-13)
    dg, du = ref.glu_grads_ref(dy, g, u, act)
    torch.testing.assert_close(dg, gd.grad, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(du, ud.grad, rtol=1e-11, atol=1e-12)


def test_oai_gradients_follow_the_clamp_convention():
    lim = ref.OAI_LIMIT
    g = torch.tensor([lim + 0.5, 100.0, lim, 6.0, -100.0, -lim], dtype=torch.float64)
    u = torch.tensor([lim + 0.5, -lim - 1, lim, -lim, 3.0, 100.0], dtype=torch.float64)
    dy = torch.ones(6, dtype=torch.float64)
    dg, du = ref.glu_grads_ref(dy, g, u, "swiglu_oai")
    assert dg[0] == 0 and dg[1] == 0 and dg[2] != 0 and dg[3] != 0          # zero beyond the bound, passed on it
    assert du[0] == 0 and du[1] == 0 and du[5] == 0 and du[2] != 0 and du[3] != 0 and du[4] != 0
    y = ref.glu_ref(g, u, "swiglu_oai")
    assert y[0] == y[2]                                      # both sides clamped to (limit, limit)
    gd, ud = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
    ref.textbook(gd, ud, "swiglu_oai").backward(dy)
    torch.testing.assert_close(dg, gd.grad, rtol=1e-12, atol=0)             # torch's own convention, bounds included
    torch.testing.assert_close(du, ud.grad, rtol=1e-12, atol=0)


@pytest.mark.parametrize("act", ref.ACTS)
def test_reference_limits_at_large_gates(act):
    g = torch.tensor([30.0, 100.0, 1e4, 65504.0], dtype=torch.float64)
    a, da = ref.act_ref(g, act)
    an, dan = ref.act_ref(-g, act)
    assert torch.isfinite(a).all() and torch.isfinite(da).all() and torch.isfinite(an).all() and torch.isfinite(dan).all()
    if act == "swiglu_oai":
        torch.testing.assert_close(a, torch.full_like(g, ref.OAI_LIMIT), rtol=1e-5, atol=0)
        assert (da == 0).all()
    else:
        # silu at g = 30 is the slowest to get there: 1 - sigmoid(30) = 9.4e-14, a' - 1 = 30 * 9.4e-14
        torch.testing.assert_close(a, g, rtol=1e-11, atol=0)
        torch.testing.assert_close(da, torch.ones_like(g), rtol=1e-11, atol=0)
    assert an.abs().max() < 1e-11 and dan.abs().max() < 1e-11


# ---- the tolerance of the GPU tests, restated ---------------------------------------------------------------------------
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.mark.parametrize("act", ref.ACTS)
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_tolerance_model(act, dt):
    """|got - ref| <= r_T |ref| + 2e-6 max|ref| with r_T = 2 u_T (16-bit: one rounding of an fp32 value plus a tie flip) or 2e-6 (fp32):
    a model that evaluates the textbook formulas in fp32 and rounds once stays inside it, on the GPU tests' input distribution"""
    gen = torch.Generator().manual_seed(7)
    g, u = (3 * torch.randn(257, 1000, generator=gen)).to(DT[dt]), (3 * torch.randn(257, 1000, generator=gen)).to(DT[dt])
    dy = torch.randn(257, 1000, generator=gen).to(DT[dt])
    gf, uf = g.float().requires_grad_(True), u.float().requires_grad_(True)
    y = ref.textbook(gf, uf, act)
    y.backward(dy.float())
    worst = max(ref.gate_ok(y.detach().to(DT[dt]), ref.glu_ref(g, u, act), dt),
                *(ref.gate_ok(t.to(DT[dt]), r, dt) for t, r in zip((gf.grad, uf.grad), ref.glu_grads_ref(dy, g, u, act))))
    print(f"{act} {dt}: worst error / gate = {worst:.3f}")
    assert worst <= 1.0, worst


# ---- the Julia shim ---------------------------------------------------------------------------------------------------
def test_shim_source_names_the_symbols():
    src = open(SHIM).read()
    for name in NEW:
        assert re.search(r"ccall\(\(:%s\b" % name, src), f"the Julia shim does not ccall {name}"
    assert re.search(r"rrule\(::typeof\(glu\)", src), "no rrule for glu in the shim"
    assert re.search(r"export [^\n]*\bglu\b", src)
    for fn in ("glu_fwd", "glu_bwd"):
        assert re.search(r"function %s\(" % fn, src), fn
    # struct GluDesc mirrors nnop_glu_desc field for field
    m = re.search(r"struct GluDesc\n(.*?)\nend", src, re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == ("dtype::Int32; act::Int32; layout::Int32; reserved::Int32 "
                                                                "rows::Int64; n::Int64; ld::Int64 alpha::Float32; limit::Float32")
