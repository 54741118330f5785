"""GPU tests of the residual add fused into RMSNorm / LayerNorm (include/nnop_hip.h, nnop_add_rms_norm and siblings).

Parity against tests/addnorm_ref.py (h rounded once on the CPU, then the fp64 formulas of oracle/naive_norms.py) over the shapes, dtype
pairs and tolerances of tests/test_norms_gpu.py -- unchanged, because the fused path rounds no more often than the two-call path they
were calibrated on.  Bitwise: the fused call IS the plain operator applied to h = x + residual (same kernel family: every base pointer
is a fresh allocation), h is torch's sum, dw / db do not depend on dh, and the in-place forms equal the out-of-place ones.

The file name sorts behind the existing GPU test files on purpose (its CPU companion is tests/test_addnorm_host.py): every existing
GPU test keeps its place in the collection order, so a run of the suite that is split by position sees the same tests in each part
as before."""
import numpy as np
import pytest
import torch

import addnorm_ref as ref
from test_norms_gpu import SHAPES, YTOL
from util import TORCH_DT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OFFSET, EPS = 0.5, 1e-5
PAIRS = [("f32", "f32"), ("f16", "f16"), ("f16", "f32"), ("bf16", "bf16"), ("bf16", "f32")]


def _np(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _t(a, dt):
    return torch.tensor(np.asarray(a, np.float32)).to(TORCH_DT[dt]).to(DEV)


def _close(got, want, dt, scale=1.0, k=1.0):
    tol = YTOL[dt]
    np.testing.assert_allclose(_np(got), want, rtol=tol["rtol"] * k, atol=tol["atol"] * k * scale)


def _inputs(n, emb, dt, wdt, seed=None):
    """x, residual ~ N(0, 2^2) + 0.5; w, b, dy, dh ~ N(0, 1)"""
    rng = np.random.default_rng(n * 7 + emb if seed is None else seed)
    return dict(x=_t(rng.standard_normal((n, emb)) * 2.0 + 0.5, dt), r=_t(rng.standard_normal((n, emb)) * 2.0 + 0.5, dt),
                w=_t(rng.standard_normal(emb), wdt), b=_t(rng.standard_normal(emb), wdt),
                dy=_t(rng.standard_normal((n, emb)), dt), dh=_t(rng.standard_normal((n, emb)), dt))


def _tolw(rdw, n, wdt):
    """the dw / db rule of tests/test_norms_gpu.py::test_shapes_and_dtypes (LayerNorm; its RMSNorm dw is the fp32 case)"""
    if wdt == "f32":
        return dict(rtol=1e-4, atol=1e-5 * np.abs(rdw).max() + 1e-6 * n)
    return dict(rtol=YTOL[wdt]["rtol"], atol=YTOL[wdt]["atol"] * max(1.0, np.abs(rdw).max()))


def _eq(a, b, what):
    assert torch.equal(a, b), f"{what}: not bitwise equal ({(a != b).sum().item()} of {a.numel()} elements differ)"


@pytest.mark.parametrize("dt,wdt", PAIRS)
@pytest.mark.parametrize("n,emb", SHAPES)
def test_parity_and_bitwise_rms(pkg, dt, wdt, n, emb):
    d = _inputs(n, emb, dt, wdt)
    x, r, w, dy, dh = d["x"], d["r"], d["w"], d["dy"], d["dh"]
    y, h, rms = pkg._add_rms_norm(x, r, w, offset=OFFSET, eps=EPS)
    ry, rh, rstd = ref.add_rms_norm_ref(x, r, _np(w), offset=OFFSET, eps=EPS)
    np.testing.assert_array_equal(_np(h), rh)
    _close(y, ry, dt, scale=np.abs(ry).max())
    np.testing.assert_allclose(_np(rms), rstd, rtol=2e-6)
    # bitwise: h is torch's sum; y and rms are the plain operator's on h
    _eq(h, x + r, "h vs torch x + residual")
    y0, rms0 = pkg._rms_norm(h, w, offset=OFFSET, eps=EPS)
    _eq(y, y0, "y vs _rms_norm(h)")
    _eq(rms, rms0, "rms vs _rms_norm(h)")
    # pullback, with and without dh
    dx0, dw0 = pkg.grad_rms_norm(dy, rms, h, w, offset=OFFSET)
    rdx, rdw = ref.add_rms_norm_grads_ref(dy, None, h, _np(w), offset=OFFSET, eps=EPS)
    for dh_ in (dh, None):
        dx, dw = pkg.grad_add_rms_norm(dy, dh_, rms, h, w, offset=OFFSET)
        want = rdx if dh_ is None else rdx + _np(dh_)
        _close(dx, want, dt, scale=np.abs(want).max())
        assert dw.dtype == torch.float32
        np.testing.assert_allclose(_np(dw), rdw, rtol=1e-4, atol=1e-5 * np.abs(rdw).max() + 1e-6 * n)
        _eq(dw, dw0, f"dw vs grad_rms_norm (dh {'given' if dh_ is not None else 'None'})")
        if dh_ is None:
            _eq(dx, dx0, "dx vs grad_rms_norm (dh None)")


@pytest.mark.parametrize("dt,wdt", PAIRS)
@pytest.mark.parametrize("n,emb", SHAPES)
def test_parity_and_bitwise_layer_norm(pkg, dt, wdt, n, emb):
    d = _inputs(n, emb, dt, wdt)
    x, r, w, b, dy, dh = d["x"], d["r"], d["w"], d["b"], d["dy"], d["dh"]
    y, h, mu, sg = pkg._add_layer_norm(x, r, w, b, eps=EPS)
    ry, rh, rmu, rsg = ref.add_layer_norm_ref(x, r, _np(w), _np(b), eps=EPS)
    np.testing.assert_array_equal(_np(h), rh)
    _close(y, ry, dt, scale=np.abs(ry).max())
    np.testing.assert_allclose(_np(mu), rmu, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(_np(sg), rsg, rtol=2e-6)
    _eq(h, x + r, "h vs torch x + residual")
    y0, mu0, sg0 = pkg._layer_norm(h, w, b, eps=EPS)
    _eq(y, y0, "y vs _layer_norm(h)")
    _eq(mu, mu0, "mu vs _layer_norm(h)")
    _eq(sg, sg0, "sigma vs _layer_norm(h)")
    dx0, dw0, db0 = pkg.grad_layer_norm(dy, mu, sg, h, w, b)
    rdx, rdw, rdb = ref.add_layer_norm_grads_ref(dy, None, h, _np(w), eps=EPS)
    for dh_ in (dh, None):
        dx, dw, db = pkg.grad_add_layer_norm(dy, dh_, mu, sg, h, w, b)
        want = rdx if dh_ is None else rdx + _np(dh_)
        _close(dx, want, dt, scale=np.abs(want).max(), k=2.0)
        assert dw.dtype == w.dtype and db.dtype == w.dtype
        np.testing.assert_allclose(_np(dw), rdw, **_tolw(rdw, n, wdt))
        np.testing.assert_allclose(_np(db), rdb, **_tolw(rdw, n, wdt))
        tag = f"(dh {'given' if dh_ is not None else 'None'})"
        _eq(dw, dw0, "dw vs grad_layer_norm " + tag)
        _eq(db, db0, "db vs grad_layer_norm " + tag)
        if dh_ is None:
            _eq(dx, dx0, "dx vs grad_layer_norm (dh None)")


@pytest.mark.parametrize("n,emb", [(5000, 128), (4100, 768)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_pullback_is_deterministic(pkg, n, emb, dt):
    """multi-partial dw / db: two runs are bitwise equal (fixed-order fold, no atomics), dx with them"""
    d = _inputs(n, emb, dt, "f32")
    _, h, rms = pkg._add_rms_norm(d["x"], d["r"], d["w"], offset=OFFSET, eps=EPS)
    a, c = (pkg.grad_add_rms_norm(d["dy"], d["dh"], rms, h, d["w"], offset=OFFSET) for _ in range(2))
    for u, v in zip(a, c):
        _eq(u, v, "grad_add_rms_norm, run 1 vs run 2")
    _, h, mu, sg = pkg._add_layer_norm(d["x"], d["r"], d["w"], d["b"], eps=EPS)
    a, c = (pkg.grad_add_layer_norm(d["dy"], d["dh"], mu, sg, h, d["w"], d["b"]) for _ in range(2))
    for u, v in zip(a, c):
        _eq(u, v, "grad_add_layer_norm, run 1 vs run 2")


# Which kernels an aliasing shape takes (csrc/row_common.hpp; every base pointer here is a fresh, aligned allocation):
#   (37, 264), (130, 2048), (33, 5000)  register kernels in both directions and both dtypes.  5000 elements are 625 (bf16) / 1250
#                                       (f32) whole 16-byte chunks: 256x4 / 256x8 forward, 1024x1 / 1024x2 pullback
#   (33, 5001)                          row bytes are no multiple of 16: the generic kernels, both directions, both dtypes
#   (5, 16392)                          past the pullback's register capacity (16 Ki elements): generic pullback in both dtypes;
#                                       the forward stays in registers (1024x4 bf16, 1024x8 f32)
#   (2, 70000)                          f32: 17500 chunks, past the forward's capacity too: generic in both directions;
#                                       bf16: the 16-chunk forward, whose residual passes through in slices; generic pullback
ALIAS_SHAPES = [(37, 264), (130, 2048), (33, 5000), (33, 5001), (5, 16392), (2, 70000)]


def test_alias_shapes_take_the_kernels_they_are_meant_to():
    """the table above, restated from the dispatch rules: a shape that silently moved to the register kernels would leave the
    in-place forms of the generic kernels (h read back from h, pointers without __restrict__) untested"""
    def chunks(emb, isz):
        return emb * isz // 16 if emb * isz % 16 == 0 else None

    def fwd_generic(emb, isz):
        return chunks(emb, isz) is None or chunks(emb, isz) > 1024 * 16

    def bwd_generic(emb, isz):
        return chunks(emb, isz) is None or chunks(emb, isz) > 1024 * (4 if isz == 4 else 2)

    for isz in (4, 2):
        for emb in (264, 2048, 5000):
            assert not fwd_generic(emb, isz) and not bwd_generic(emb, isz)
        assert fwd_generic(5001, isz) and bwd_generic(5001, isz)
        assert not fwd_generic(16392, isz) and bwd_generic(16392, isz)
        assert bwd_generic(70000, isz)
    assert fwd_generic(70000, 4) and not fwd_generic(70000, 2) and chunks(70000, 2) > 1024 * 8


@pytest.mark.parametrize("n,emb", ALIAS_SHAPES)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_in_place_forms_equal_the_out_of_place_call(pkg, n, emb, dt):
    d = _inputs(n, emb, dt, "f32")
    x, r, w, b, dy, dh = d["x"], d["r"], d["w"], d["b"], d["dy"], d["dh"]
    want = pkg._add_rms_norm(x, r, w, offset=OFFSET, eps=EPS)
    want_ln = pkg._add_layer_norm(x, r, w, b, eps=EPS)
    for which in ("x", "residual"):
        for op, base in (("rms", want), ("ln", want_ln)):
            xc, rc = x.clone(), r.clone()
            buf = xc if which == "x" else rc
            got = (pkg._add_rms_norm(xc, rc, w, offset=OFFSET, eps=EPS, h_out=buf) if op == "rms"
                   else pkg._add_layer_norm(xc, rc, w, b, eps=EPS, h_out=buf))
            assert got[1] is buf and got[1].data_ptr() == buf.data_ptr()
            for u, v, name in zip(got, base, ("y", "h", "stat0", "stat1")):
                _eq(u, v, f"{op} h_out is {which}: {name}")
            # the other input is untouched
            _eq(rc if which == "x" else xc, r if which == "x" else x, f"{op} h_out is {which}: the other input")
    y, h, rms = want
    base = pkg.grad_add_rms_norm(dy, dh, rms, h, w, offset=OFFSET)
    dhc = dh.clone()
    got = pkg.grad_add_rms_norm(dy, dhc, rms, h, w, offset=OFFSET, dx_out=dhc)
    assert got[0] is dhc
    for u, v, name in zip(got, base, ("dx", "dw")):
        _eq(u, v, f"rms dx_out is dh: {name}")
    y, h, mu, sg = want_ln
    base = pkg.grad_add_layer_norm(dy, dh, mu, sg, h, w, b)
    dhc = dh.clone()
    got = pkg.grad_add_layer_norm(dy, dhc, mu, sg, h, w, b, dx_out=dhc)
    assert got[0] is dhc
    for u, v, name in zip(got, base, ("dx", "dw", "db")):
        _eq(u, v, f"ln dx_out is dh: {name}")


def _misaligned(t):
    """the same values as a contiguous view that starts one element into a flat buffer: its base is not 16-byte aligned"""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0 and t.data_ptr() % 16 == 0
    return v


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("which", ["x", "residual", "dh"])
def test_misaligned_bases_take_the_generic_kernel(pkg, dt, which):
    """rows of (64, 520) fit the register kernels; a base that is not 16-byte aligned must send the call to the element-wise kernel
    (a 16-byte access at such an address faults or reads the wrong bytes).  Results within the parity tolerances."""
    n, emb = 64, 520
    d = _inputs(n, emb, dt, "f32")
    x, r, w, b, dy, dh = d["x"], d["r"], d["w"], d["b"], d["dy"], d["dh"]
    xm = _misaligned(x) if which == "x" else x
    rm = _misaligned(r) if which == "residual" else r
    dhm = _misaligned(dh) if which == "dh" else dh
    ry, rh, rstd = ref.add_rms_norm_ref(x, r, _np(w), offset=OFFSET, eps=EPS)
    y, h, rms = pkg._add_rms_norm(xm, rm, w, offset=OFFSET, eps=EPS)
    np.testing.assert_array_equal(_np(h), rh)
    _close(y, ry, dt, scale=np.abs(ry).max())
    np.testing.assert_allclose(_np(rms), rstd, rtol=2e-6)
    rdx, rdw = ref.add_rms_norm_grads_ref(dy, dh, h, _np(w), offset=OFFSET, eps=EPS)
    dx, dw = pkg.grad_add_rms_norm(dy, dhm, rms, h, w, offset=OFFSET)
    _close(dx, rdx, dt, scale=np.abs(rdx).max())
    np.testing.assert_allclose(_np(dw), rdw, rtol=1e-4, atol=1e-5 * np.abs(rdw).max() + 1e-6 * n)
    ry, rh, rmu, rsg = ref.add_layer_norm_ref(x, r, _np(w), _np(b), eps=EPS)
    y, h, mu, sg = pkg._add_layer_norm(xm, rm, w, b, eps=EPS)
    np.testing.assert_array_equal(_np(h), rh)
    _close(y, ry, dt, scale=np.abs(ry).max())
    np.testing.assert_allclose(_np(mu), rmu, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(_np(sg), rsg, rtol=2e-6)
    rdx, rdw, rdb = ref.add_layer_norm_grads_ref(dy, dh, h, _np(w), eps=EPS)
    dx, dw, db = pkg.grad_add_layer_norm(dy, dhm, mu, sg, h, w, b)
    _close(dx, rdx, dt, scale=np.abs(rdx).max(), k=2.0)
    np.testing.assert_allclose(_np(dw), rdw, **_tolw(rdw, n, "f32"))
    np.testing.assert_allclose(_np(db), rdb, **_tolw(rdw, n, "f32"))


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_misaligned_x_of_the_plain_operators(pkg, dt):
    from oracle.naive_norms import naive_layer_norm, naive_rms_norm
    n, emb = 64, 520
    d = _inputs(n, emb, dt, "f32")
    xm, w, b = _misaligned(d["x"]), d["w"], d["b"]
    y, rms = pkg._rms_norm(xm, w, offset=OFFSET, eps=EPS)
    ry, rstd = naive_rms_norm(_np(d["x"]), _np(w), offset=OFFSET, eps=EPS)
    _close(y, ry, dt, scale=np.abs(ry).max())
    np.testing.assert_allclose(_np(rms), rstd, rtol=2e-6)
    y, mu, sg = pkg._layer_norm(xm, w, b, eps=EPS)
    ry, rmu, rsg = naive_layer_norm(_np(d["x"]), _np(w), _np(b), eps=EPS)
    _close(y, ry, dt, scale=np.abs(ry).max())
    np.testing.assert_allclose(_np(mu), rmu, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(_np(sg), rsg, rtol=2e-6)


@pytest.mark.parametrize("op", ["rms", "ln"])
def test_autograd_matches_torch_double(pkg, op):
    rng = np.random.default_rng(3)
    n, emb = 33, 777
    mk = lambda *s: _t(rng.standard_normal(s), "f32")
    x, r, w, b = (mk(n, emb).requires_grad_(True), mk(n, emb).requires_grad_(True), mk(emb).requires_grad_(True),
                  mk(emb).requires_grad_(True))
    g1, g2 = mk(n, emb), mk(n, emb)
    F = torch.nn.functional
    if op == "rms":
        fused = lambda: pkg.add_rms_norm(x, r, w, eps=1e-5)
        params, pd_of = (w,), lambda wd, bd: (wd,)
        plain = lambda hd, wd, bd: F.rms_norm(hd, (emb,), wd, eps=1e-5)
    else:
        fused = lambda: pkg.add_layer_norm(x, r, w, b, eps=1e-5)
        params, pd_of = (w, b), lambda wd, bd: (wd, bd)
        plain = lambda hd, wd, bd: F.layer_norm(hd, (emb,), wd, bd, eps=1e-5)

    def clear():
        for t in (x, r, w, b):
            t.grad = None

    def double_grads(use_y, use_h):
        xd, rd, wd, bd = (t.detach().double().requires_grad_(True) for t in (x, r, w, b))
        hd = xd + rd
        loss = 0.0
        if use_y:
            loss = loss + (plain(hd, wd, bd) * g1.double()).sum()
        if use_h:
            loss = loss + (hd * g2.double()).sum()
        loss.backward()
        return xd.grad, rd.grad, [p.grad for p in pd_of(wd, bd)]

    # both outputs
    y, h = fused()
    assert not y.data_ptr() == x.data_ptr() and not h.data_ptr() in (x.data_ptr(), r.data_ptr())      # never in place
    ((y * g1).sum() + (h * g2).sum()).backward()
    xg, rg, pg = double_grads(True, True)
    assert torch.equal(x.grad, r.grad)
    np.testing.assert_allclose(_np(x.grad), _np(xg), rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(_np(r.grad), _np(rg), rtol=2e-4, atol=2e-5)
    for p, q in zip(params, pg):
        np.testing.assert_allclose(_np(p.grad), _np(q), rtol=2e-4, atol=2e-5)
    # y alone: h unused reaches the library as dh = NULL
    clear()
    y, h = fused()
    (y * g1).sum().backward()
    xg, rg, pg = double_grads(True, False)
    assert torch.equal(x.grad, r.grad)
    np.testing.assert_allclose(_np(x.grad), _np(xg), rtol=2e-4, atol=2e-5)
    for p, q in zip(params, pg):
        np.testing.assert_allclose(_np(p.grad), _np(q), rtol=2e-4, atol=2e-5)
    # h alone: the add by itself; the parameters get zeros
    clear()
    y, h = fused()
    (h * g2).sum().backward()
    assert torch.equal(x.grad, g2) and torch.equal(r.grad, g2)
    for p in params:
        assert p.grad is None or not p.grad.any()
    # no grad: the same values
    with torch.no_grad():
        y2, h2 = fused()
    assert torch.equal(y2, y) and torch.equal(h2, h)
