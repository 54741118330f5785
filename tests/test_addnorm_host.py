"""CPU tests of the residual add fused into RMSNorm / LayerNorm (include/nnop_hip.h, nnop_add_rms_norm and its three siblings): the
four entry points are declared, bound and exported; they validate as the plain norm entry points do and return before any launch; the
Python wrappers refuse CPU tensors and a mismatched residual; and the reference the GPU tests are judged against (tests/addnorm_ref.py)
has the right gradient -- one array, for x and for residual alike."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import addnorm_ref as ref
from abi_util import HEADER, SHIM, strip_c_comments
from oracle.naive_norms import naive_layer_norm, naive_rms_norm

NEW = ("nnop_add_rms_norm", "nnop_add_rms_norm_bwd", "nnop_add_layer_norm", "nnop_add_layer_norm_bwd")


def test_exports(pkg):
    header = strip_c_comments(open(HEADER).read())
    declared = set(re.findall(r"\b(nnop_[a-z_]+)\s*\(", header))
    lib = pkg._lib.load()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/nnop_hip.h"
        assert name in pkg._lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert getattr(lib, name).argtypes is not None
    assert lib.nnop_abi_version() == 7 and pkg._lib.ABI_VERSION == 7


def _calls(lib, d, p, ws_bytes):
    """the four entry points with every pointer = p (dh included) and a workspace of ws_bytes"""
    f = C.c_float(0.0)
    return [lib.nnop_add_rms_norm(C.byref(d), p, p, p, p, p, p, f, f, None),
            lib.nnop_add_rms_norm_bwd(C.byref(d), p, p, p, p, p, p, p, f, p, ws_bytes, None),
            lib.nnop_add_layer_norm(C.byref(d), p, p, p, p, p, p, p, p, f, None),
            lib.nnop_add_layer_norm_bwd(C.byref(d), p, p, p, p, p, p, p, p, p, p, ws_bytes, None)]


@pytest.mark.parametrize("kw,status", [
    (dict(dtype=9), "NNOP_ERR_DTYPE"),
    (dict(dtype=0, w_dtype=2), "NNOP_ERR_DTYPE"),       # w must be fp32 or T
    (dict(emb=0), "NNOP_ERR_SHAPE"),
    (dict(n=0), "NNOP_ERR_SHAPE"),
    (dict(reserved=1), "NNOP_ERR_SHAPE"),
    (dict(), "NNOP_ERR_NULL"),
])
def test_descriptor_validation(pkg, kw, status):
    """the table of tests/test_norms.py::test_norm_descriptor_validation: same codes, descriptor before pointers"""
    base = dict(dtype=2, w_dtype=0, emb=1024, reserved=0, n=64)
    base.update(kw)
    d = pkg._lib.NormDesc(**base)
    want = getattr(pkg._lib, status)
    assert _calls(pkg._lib.load(), d, C.c_void_p(0), 0) == [want] * 4


def test_null_and_workspace_checks_come_before_any_launch(pkg):
    lib = pkg._lib.load()
    d = pkg._lib.NormDesc(dtype=2, w_dtype=0, emb=1024, reserved=0, n=64)
    ok = C.c_void_p(0x7f0000001000)                      # never dereferenced: every call below returns before a launch
    f = C.c_float(0.0)
    need = lib.nnop_norm_bwd_workspace_bytes(C.byref(d), 0)
    assert need > 0 and lib.nnop_norm_bwd_workspace_bytes(C.byref(d), 1) == 2 * need
    # all pointers non-NULL, workspace one byte short
    st = _calls(lib, d, ok, need - 1)
    assert st[1] == pkg._lib.NNOP_ERR_WORKSPACE and st[3] == pkg._lib.NNOP_ERR_WORKSPACE
    assert lib.nnop_add_layer_norm_bwd(C.byref(d), ok, ok, ok, ok, ok, ok, ok, ok, ok, ok, 2 * need - 1, None) == pkg._lib.NNOP_ERR_WORKSPACE
    # dh is the one pointer that may be NULL: with it NULL the size check is still reached ...
    assert lib.nnop_add_rms_norm_bwd(C.byref(d), ok, ok, ok, None, ok, ok, ok, f, ok, 0, None) == pkg._lib.NNOP_ERR_WORKSPACE
    assert lib.nnop_add_layer_norm_bwd(C.byref(d), ok, ok, ok, ok, None, ok, ok, ok, ok, ok, 0, None) == pkg._lib.NNOP_ERR_WORKSPACE
    # ... while any other NULL pointer is refused first, whatever the workspace
    for pos in range(7):
        if pos == 3:
            continue
        a = [ok] * 7
        a[pos] = None
        assert lib.nnop_add_rms_norm_bwd(C.byref(d), *a, f, ok, 0, None) == pkg._lib.NNOP_ERR_NULL, pos
    for pos in range(9):
        if pos == 4:
            continue
        a = [ok] * 9
        a[pos] = None
        assert lib.nnop_add_layer_norm_bwd(C.byref(d), *a, ok, 0, None) == pkg._lib.NNOP_ERR_NULL, pos
    for pos in range(6):
        a = [ok] * 6
        a[pos] = None
        assert lib.nnop_add_rms_norm(C.byref(d), *a, f, f, None) == pkg._lib.NNOP_ERR_NULL, pos
    for pos in range(8):
        a = [ok] * 8
        a[pos] = None
        assert lib.nnop_add_layer_norm(C.byref(d), *a, f, None) == pkg._lib.NNOP_ERR_NULL, pos
    assert lib.nnop_add_rms_norm_bwd(C.byref(d), ok, ok, ok, ok, ok, ok, ok, f, None, 1 << 30, None) == pkg._lib.NNOP_ERR_NULL


def test_python_checks(pkg):
    x, w = torch.ones(4, 32), torch.ones(32)
    for call in (lambda: pkg.add_rms_norm(x, x, w), lambda: pkg._add_rms_norm(x, x, w),
                 lambda: pkg.add_layer_norm(x, x, w, w), lambda: pkg._add_layer_norm(x, x, w, w),
                 lambda: pkg.grad_add_rms_norm(x, x, torch.ones(4), x, w),
                 lambda: pkg.grad_add_layer_norm(x, None, torch.ones(4), torch.ones(4), x, w, w)):
        with pytest.raises(pkg.NNopError, match="GPU-only"):
            call()
    assert pkg.workmodel.add_norm_bytes(1024, 1024, 2) == 8 * 2 ** 20 == pkg.workmodel.add_norm_bytes(1024, 1024, 2, bwd=True)


def test_residual_mismatch_is_a_type_error(pkg):
    """`residual` of another shape or dtype raises TypeError.  The host checks run in front of any device work, so CPU tensors that
    claim to be on the GPU reach them."""
    class OnGpu(torch.Tensor):
        is_cuda = True

    mk = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt).as_subclass(OnGpu)
    x, w = mk(4, 32), mk(32)
    for bad in (mk(4, 31), mk(5, 32), mk(4, 32, dt=torch.float16), mk(32)):
        with pytest.raises(TypeError, match="residual"):
            pkg._add_rms_norm(x, bad, w)
        with pytest.raises(TypeError, match="residual"):
            pkg._add_layer_norm(x, bad, w, w)
        with pytest.raises(TypeError, match="residual"):
            pkg.add_rms_norm(x.clone().requires_grad_(True), bad, w)
    with pytest.raises(TypeError, match="dy"):
        pkg.grad_add_rms_norm(mk(4, 31), None, torch.ones(4), x, w)
    with pytest.raises(TypeError, match="dh"):
        pkg.grad_add_layer_norm(x, mk(4, 32, dt=torch.float16), torch.ones(4), torch.ones(4), x, w, w)


def _fd(f, a, idx, eps=1e-6):
    p, m = a.copy(), a.copy()
    p[idx] += eps
    m[idx] -= eps
    return (f(p) - f(m)) / (2 * eps)


@pytest.mark.parametrize("offset", [0.0, 1.0])
def test_reference_rms_gradient_matches_finite_differences(offset):
    """shapes and bounds of tests/test_norms.py::test_rms_norm_grads_match_finite_differences; fp64, so T(x + r) is x + r"""
    rng = np.random.default_rng(0)
    x, r, w = rng.random((5, 33)), rng.random((5, 33)), rng.random(33)
    dy, dh = rng.standard_normal((5, 33)), rng.standard_normal((5, 33))
    xt, rt = torch.tensor(x), torch.tensor(r)
    y, h, _ = ref.add_rms_norm_ref(xt, rt, w, offset=offset)
    np.testing.assert_array_equal(h, x + r)
    np.testing.assert_array_equal(y, naive_rms_norm(x + r, w, offset=offset)[0])
    dx, dw = ref.add_rms_norm_grads_ref(dy, dh, h, w, offset=offset)

    def loss_x(xx):
        hh = xx + r
        return (naive_rms_norm(hh, w, offset=offset)[0] * dy).sum() + (hh * dh).sum()

    def loss_r(rr):
        hh = x + rr
        return (naive_rms_norm(hh, w, offset=offset)[0] * dy).sum() + (hh * dh).sum()

    for idx in [(0, 0), (2, 17), (4, 32)]:
        assert abs(_fd(loss_x, x, idx) - dx[idx]) < 1e-7
        assert abs(_fd(loss_r, r, idx) - dx[idx]) < 1e-7           # the gradient of residual is the same array
    loss_w = lambda ww: (naive_rms_norm(x + r, ww, offset=offset)[0] * dy).sum()
    for idx in [0, 16, 32]:
        assert abs(_fd(loss_w, w, idx) - dw[idx]) < 1e-7
    dx0, _ = ref.add_rms_norm_grads_ref(dy, None, h, w, offset=offset)
    np.testing.assert_array_equal(dx0 + dh, dx)


def test_reference_layer_norm_gradient_matches_finite_differences():
    """shapes and bounds of tests/test_norms.py::test_layer_norm_grads_match_finite_differences"""
    rng = np.random.default_rng(1)
    x, r, w, b = rng.random((4, 29)), rng.random((4, 29)), rng.random(29), rng.random(29)
    dy, dh = rng.standard_normal((4, 29)), rng.standard_normal((4, 29))
    y, h, _, _ = ref.add_layer_norm_ref(torch.tensor(x), torch.tensor(r), w, b)
    np.testing.assert_array_equal(h, x + r)
    dx, dw, db = ref.add_layer_norm_grads_ref(dy, dh, h, w)

    def loss_x(xx):
        hh = xx + r
        return (naive_layer_norm(hh, w, b)[0] * dy).sum() + (hh * dh).sum()

    def loss_r(rr):
        hh = x + rr
        return (naive_layer_norm(hh, w, b)[0] * dy).sum() + (hh * dh).sum()

    for idx in [(0, 0), (1, 13), (3, 28)]:
        assert abs(_fd(loss_x, x, idx) - dx[idx]) < 1e-6
        assert abs(_fd(loss_r, r, idx) - dx[idx]) < 1e-6
    for idx in [0, 14, 28]:
        assert abs(_fd(lambda ww: (naive_layer_norm(x + r, ww, b)[0] * dy).sum(), w, idx) - dw[idx]) < 1e-7
        assert abs(_fd(lambda bb: (naive_layer_norm(x + r, w, bb)[0] * dy).sum(), b, idx) - db[idx]) < 1e-7


def test_reference_rounds_h_once():
    """h = T(fp32(x) + fp32(r)): one rounding, and the statistics are those of the rounded h"""
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(7, 40, generator=g) * 2 + 0.5).to(torch.bfloat16)
    r = (torch.randn(7, 40, generator=g) * 2 + 0.5).to(torch.bfloat16)
    h = ref.add_h(x, r)
    assert h.dtype == torch.bfloat16 and torch.equal(h, x + r)
    y, hh, rstd = ref.add_rms_norm_ref(x, r, np.ones(40))
    np.testing.assert_array_equal(hh, h.double().numpy())
    np.testing.assert_allclose(rstd, 1 / np.sqrt((hh * hh).mean(-1) + 1e-6), rtol=1e-14)
    assert np.abs(hh - (x.double() + r.double()).numpy()).max() > 0          # the rounding is visible: the exact sum differs


def test_shim_source_names_the_symbols():
    src = open(SHIM).read()
    for name in NEW:
        assert re.search(r":%s\b" % name, src), f"the Julia shim does not ccall {name}"
    for fn in ("add_rms_norm", "add_layer_norm"):
        assert re.search(r"rrule\(::typeof\((NNop\.)?%s\)" % fn, src), f"no rrule for {fn} in the shim"
