"""GPU tests of the gated MLP activations (include/nnop_hip.h, nnop_glu / nnop_glu_bwd; nnop.jl_amd/activations.py).

Parity against tests/glu_ref.py (fp64 on the rounded inputs) at the derived tolerance |got - ref| <= r_T |ref| + 2e-6 max|ref|, r_T = 2 u_T for
the 16-bit types (one rounding of an fp32 value plus a tie flip) and 2e-6 for fp32 (tests/test_z_glu_host.py::test_tolerance_model restates
it on the CPU).  Bitwise: every layout, the 16-byte and the element-wise path, a padded row stride and the in-place forms compute one and
the same function of (gate, up, dy) -- any difference is an addressing bug.  Shapes are chosen for where the indexing can break, not for
size; the whole file runs in a few seconds.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import functools
import itertools

import pytest
import torch

import glu_ref as ref
from util import TORCH_DT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = ("f32", "f16", "bf16")
LAYOUTS = ("dense", "halves", "interleaved")
# (1, 1), (3, 40), (37, 264)  one element; narrow vector rows; lanes crossing row ends
# (5, 1003)                   odd n: the element-wise path; packed halves: the base of `up` is misaligned
# (7, 1004)                   n % 8 = 4: 16-bit element-wise, fp32 vector
# (4100, 24)                  many short rows, several workgroups
# (2, 70000)                  long rows
# (130, 2048)                 the plain vector case
SHAPES = [(1, 1), (3, 40), (37, 264), (5, 1003), (7, 1004), (4100, 24), (2, 70000), (130, 2048)]


@functools.lru_cache(maxsize=None)
def _cpu_inputs(rows, n, dt):
    """gate, up ~ 3 N(0, 1), dy ~ N(0, 1), rounded to the element type, on the CPU; seeded by the shape"""
    gen = torch.Generator().manual_seed(rows * 100003 + n)
    g = (3 * torch.randn(rows, n, generator=gen)).to(TORCH_DT[dt])
    u = (3 * torch.randn(rows, n, generator=gen)).to(TORCH_DT[dt])
    dy = torch.randn(rows, n, generator=gen).to(TORCH_DT[dt])
    return g, u, dy


@functools.lru_cache(maxsize=None)
def _reference(rows, n, dt, act):
    g, u, dy = _cpu_inputs(rows, n, dt)
    return (ref.glu_ref(g, u, act), *ref.glu_grads_ref(dy, g, u, act))


def _gpu_inputs(rows, n, dt):
    return tuple(t.to(DEV) for t in _cpu_inputs(rows, n, dt))


def _eq(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), f"{what}: not bitwise equal ({(a != b).sum().item()} of {a.numel()} elements differ)"


def _run(pkg, layout, act, g, u, dy):
    """(y, dgate, dup) through one layout; every tensor that reaches the library is a fresh allocation"""
    n = g.shape[-1]
    if layout == "dense":
        return (pkg._glu(g, u, act=act), *pkg.grad_glu(dy, g, u, act=act))
    if layout == "halves":                       # the two halves of one fused projection, by stride: up = base + n, ld = 2n
        gu = torch.cat((g, u), dim=-1)
        gate, up = gu.chunk(2, dim=-1)
        assert gate.data_ptr() == gu.data_ptr() and up.data_ptr() == gu.data_ptr() + n * gu.element_size()
        y = pkg._glu(gate, up, act=act)
        _eq(pkg.glu_packed(gu, act=act, layout="halves"), y, "glu_packed(halves) vs the chunk views")
        dgu = pkg.grad_glu_packed(dy, gu, act=act, layout="halves")
        dgate, dup = pkg.grad_glu(dy, gate, up, act=act)
        _eq(dgu[..., :n], dgate, "grad_glu_packed(halves) dgate vs the chunk views")
        _eq(dgu[..., n:], dup, "grad_glu_packed(halves) dup vs the chunk views")
        return y, dgate.contiguous(), dup.contiguous()
    gu = ref.interleave(g, u)
    y = pkg.glu_packed(gu, act=act, layout="interleaved")
    dgu = pkg.grad_glu_packed(dy, gu, act=act, layout="interleaved")
    assert dgu.shape == gu.shape
    return y, dgu[..., 0::2].contiguous(), dgu[..., 1::2].contiguous()


def _parity_cases():
    """every activation x layout x dtype at two shapes, every shape with every layout: a Latin square over pairs of shapes"""
    out = []
    for (li, layout), (di, dt), (ai, act) in itertools.product(enumerate(LAYOUTS), enumerate(DTS), enumerate(ref.ACTS)):
        k = (ai + di + li) % 4
        out += [(layout, dt, act, SHAPES[2 * k]), (layout, dt, act, SHAPES[2 * k + 1])]
    return out


def test_parity_cases_cover_what_they_should():
    cases = _parity_cases()
    for combo in itertools.product(LAYOUTS, DTS, ref.ACTS):
        assert sum(c[:3] == combo for c in cases) >= 2, combo
    for layout, shape in itertools.product(LAYOUTS, SHAPES):
        assert any(c[0] == layout and c[3] == shape for c in cases), (layout, shape)
    for dt, shape in itertools.product(DTS, SHAPES):
        assert any(c[1] == dt and c[3] == shape for c in cases), (dt, shape)


@pytest.mark.parametrize("layout,dt,act,shape", _parity_cases())
def test_parity(pkg, layout, dt, act, shape):
    g, u, dy = _gpu_inputs(*shape, dt)
    got = _run(pkg, layout, act, g, u, dy)
    for name, t, r in zip(("y", "dgate", "dup"), got, _reference(*shape, dt, act)):
        assert t.dtype == TORCH_DT[dt] and tuple(t.shape) == shape
        worst = ref.gate_ok(t, r, dt)
        print(f"{layout} {dt} {act} {shape} {name}: worst error / gate = {worst:.3f}")
        assert worst <= 1.0, f"{name}: error is {worst:.3f} of the gate"


def _misaligned(t):
    """the same values as a contiguous view that starts one element into a flat buffer: its base is not 16-byte aligned"""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0 and t.data_ptr() % 16 == 0
    return v


def _padded(t, pad, fill):
    """the same values as a view [rows, n] of a [rows, n + pad] buffer whose padding holds `fill`"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=t.device)
    v = buf[:, :t.shape[1]]
    v.copy_(t)
    return buf, v


@pytest.mark.parametrize("si,di", list(itertools.product(range(len(SHAPES)), range(len(DTS)))))
def test_bitwise_identities(pkg, si, di):
    shape, dt, act = SHAPES[si], DTS[di], ref.ACTS[(si + di) % 4]
    rows, n = shape
    g, u, dy = _gpu_inputs(*shape, dt)
    base = _run(pkg, "dense", act, g, u, dy)
    names = ("y", "dgate", "dup")
    # the three layouts, and a second run
    for layout in ("halves", "interleaved", "dense"):
        for name, a, b in zip(names, _run(pkg, layout, act, g, u, dy), base):
            _eq(a, b, f"{layout} vs dense ({act} {dt} {shape}): {name}")
    # a base misaligned by one element, one argument at a time: the element-wise path computes the same bits
    for which in ("gate", "up", "dy", "out"):
        gm = _misaligned(g) if which == "gate" else g
        um = _misaligned(u) if which == "up" else u
        dym = _misaligned(dy) if which == "dy" else dy
        if which == "out":
            y = pkg.glu_into(_misaligned(torch.empty_like(g)), g, u, act=act)
            dgate, dup = pkg.grad_glu_into(_misaligned(torch.empty_like(g)), torch.empty_like(u), dy, g, u, act=act)
        else:
            y = pkg._glu(gm, um, act=act)
            dgate, dup = pkg.grad_glu(dym, gm, um, act=act)
        for name, a, b in zip(names, (y, dgate, dup), base):
            _eq(a, b, f"misaligned {which} vs aligned ({act} {dt} {shape}): {name}")
    gum = _misaligned(ref.interleave(g, u))
    _eq(pkg.glu_packed(gum, act=act, layout="interleaved"), base[0], "misaligned gu vs dense: y")
    dgu = pkg.grad_glu_packed(dy, gum, act=act, layout="interleaved")
    _eq(dgu[..., 0::2], base[1], "misaligned gu vs dense: dgate")
    _eq(dgu[..., 1::2], base[2], "misaligned gu vs dense: dup")
    # a split call with ld = n + 8: the same results, and the padding of dgate / dup keeps its sentinel
    (_, gp), (_, up_) = _padded(g, 8, 1.0), _padded(u, 8, 1.0)
    assert pkg.activations._row_stride(gp) == n + 8 or rows == 1
    _eq(pkg._glu(gp, up_, act=act), base[0], "ld = n + 8 vs dense: y")
    (dgbuf, dgv), (dubuf, duv) = _padded(torch.zeros_like(g), 8, -77.0), _padded(torch.zeros_like(u), 8, -77.0)
    pkg.grad_glu_into(dgv, duv, dy, gp, up_, act=act)
    _eq(dgv, base[1], "ld = n + 8 vs dense: dgate")
    _eq(duv, base[2], "ld = n + 8 vs dense: dup")
    assert (dgbuf[:, n:] == -77.0).all() and (dubuf[:, n:] == -77.0).all(), "the padding between n and ld was written"
    dgate, dup = pkg.grad_glu(dy, gp, up_, act=act)           # fresh gradients take the inputs' strides
    assert dgate.stride() == gp.stride() or rows == 1
    _eq(dgate, base[1], "ld = n + 8, fresh gradients: dgate")
    _eq(dup, base[2], "ld = n + 8, fresh gradients: dup")


@pytest.mark.parametrize("shape", [(130, 2048), (5, 1003)])       # the 16-byte path; the element-wise path
@pytest.mark.parametrize("ai,dt", [(0, "bf16"), (1, "f32"), (2, "f16"), (3, "bf16"), (3, "f32")])
def test_in_place_forms_equal_the_out_of_place_call(pkg, shape, ai, dt):
    act = ref.ACTS[ai]
    n = shape[1]
    g, u, dy = _gpu_inputs(*shape, dt)
    y0 = pkg._glu(g, u, act=act)
    dg0, du0 = pkg.grad_glu(dy, g, u, act=act)
    # y over gate, y over up: the other input is untouched
    gc, uc = g.clone(), u.clone()
    assert pkg.glu_into(gc, gc, uc, act=act) is gc
    _eq(gc, y0, "y over gate")
    _eq(uc, u, "y over gate: up")
    gc, uc = g.clone(), u.clone()
    assert pkg.glu_into(uc, gc, uc, act=act) is uc
    _eq(uc, y0, "y over up")
    _eq(gc, g, "y over up: gate")
    # dgate over gate and dup over up, together and one at a time
    gc, uc, dyc = g.clone(), u.clone(), dy.clone()
    a, b = pkg.grad_glu_into(gc, uc, dyc, gc, uc, act=act)
    assert a is gc and b is uc
    _eq(gc, dg0, "dgate over gate")
    _eq(uc, du0, "dup over up")
    _eq(dyc, dy, "in-place pullback: dy")
    gc, uc = g.clone(), u.clone()
    _, dup = pkg.grad_glu_into(gc, torch.empty_like(u), dy, gc, uc, act=act)
    _eq(gc, dg0, "dgate over gate alone")
    _eq(dup, du0, "dgate over gate alone: dup")
    _eq(uc, u, "dgate over gate alone: up")
    # dgu over gu, both packed layouts
    for layout, gu in (("halves", torch.cat((g, u), -1)), ("interleaved", ref.interleave(g, u))):
        want = pkg.grad_glu_packed(dy, gu, act=act, layout=layout)
        guc = gu.clone()
        assert pkg.grad_glu_packed(dy, guc, act=act, layout=layout, dgu_out=guc) is guc
        _eq(guc, want, f"dgu over gu ({layout})")
        dgate, dup = (want[..., :n], want[..., n:]) if layout == "halves" else (want[..., 0::2], want[..., 1::2])
        _eq(dgate, dg0, f"{layout}: dgate")
        _eq(dup, du0, f"{layout}: dup")
    # the halves of one projection, in place through the views
    guc = torch.cat((g, u), -1)
    gv, uv = guc.chunk(2, -1)
    pkg.grad_glu_into(gv, uv, dy, gv, uv, act=act)
    _eq(guc, torch.cat((dg0, du0), -1), "dgate / dup over the chunk views of gu")


EXTREME = (30.0, 100.0, 1e4, 65504.0)


@pytest.mark.parametrize("act", ref.ACTS)
@pytest.mark.parametrize("dt", DTS)
def test_extreme_finite_gates(pkg, dt, act):
    """gate in {+-30, +-100, +-1e4, +-65504}, one value per row, with ordinary up and dy.  fp16's largest finite number is 65504, so
    y = a * up and dup = dy * a at a = 65504 are finite only for |up|, |dy| < 1: up, dy ~ 0.25 N(0, 1) clipped to +-0.9, for every dtype."""
    T = TORCH_DT[dt]
    n = 72
    gen = torch.Generator().manual_seed(11)
    vals = [s * v for v in EXTREME for s in (1.0, -1.0)]
    g = torch.tensor(vals).repeat_interleave(n).view(len(vals), n).to(T)
    u = (0.25 * torch.randn(len(vals), n, generator=gen)).clamp(-0.9, 0.9).to(T)
    dy = (0.25 * torch.randn(len(vals), n, generator=gen)).clamp(-0.9, 0.9).to(T)
    want = (ref.glu_ref(g, u, act), *ref.glu_grads_ref(dy, g, u, act))
    gd, ud, dyd = g.to(DEV), u.to(DEV), dy.to(DEV)
    pos, neg = slice(0, None, 2), slice(1, None, 2)
    for layout in ("dense", "interleaved"):
        got = _run(pkg, layout, act, gd, ud, dyd)
        for name, t, r in zip(("y", "dgate", "dup"), got, want):
            assert torch.isfinite(t).all(), f"{layout} {name}: not finite"
            assert ref.gate_ok(t, r, dt) <= 1.0, f"{layout} {name}: error is {ref.gate_ok(t, r, dt):.3f} of the gate"
        y, dgate, dup = (ref.f64(t) for t in got)
        G, U, DY = ref.f64(g), ref.f64(u), ref.f64(dy)
        rt = ref.R_T[dt]
        # large negative gates: a -> 0 and a' -> 0 (silu at -30 is the slowest: 30 e^-30 = 2.8e-12)
        assert y[neg].abs().max() <= 1e-11 and dgate[neg].abs().max() <= 1e-11 and dup[neg].abs().max() <= 1e-11
        if act == "swiglu_oai":
            # clamped at the limit: a = limit sigmoid(alpha limit), and no gradient reaches a gate beyond it
            a = ref.OAI_LIMIT * torch.sigmoid(torch.tensor(ref.OAI_ALPHA * ref.OAI_LIMIT, dtype=torch.float64))
            assert (dgate[pos] == 0).all()
            assert ((y[pos] - a * (U[pos] + 1)).abs() <= 2 * rt * (a * (U[pos] + 1)).abs()).all()
            assert ((dup[pos] - DY[pos] * a).abs() <= 2 * rt * (DY[pos] * a).abs()).all()
        else:
            # large positive gates: a -> g, a' -> 1, to within the rounding of the result
            assert ((y[pos] - G[pos] * U[pos]).abs() <= 2 * rt * (G[pos] * U[pos]).abs()).all()
            assert ((dup[pos] - DY[pos] * G[pos]).abs() <= 2 * rt * (DY[pos] * G[pos]).abs()).all()
            assert ((dgate[pos] - DY[pos] * U[pos]).abs() <= 2 * rt * (DY[pos] * U[pos]).abs()).all()


# ---- autograd ------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().double().cpu().numpy()


def _close(a, b):
    import numpy as np
    np.testing.assert_allclose(_np(a), _np(b), rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("which", ["swiglu", "geglu_tanh", "geglu_none", "packed_halves", "packed_interleaved"])
def test_autograd_matches_torch_double(pkg, which):
    rows, n = 33, 777
    gen = torch.Generator().manual_seed(3)
    g0, u0, dy = (torch.randn(rows, n, generator=gen).to(DEV) for _ in range(3))
    g0, u0 = 3 * g0, 3 * u0
    act = {"swiglu": "silu", "geglu_tanh": "gelu_tanh", "geglu_none": "gelu_erf", "packed_halves": "gelu_tanh",
           "packed_interleaved": "swiglu_oai"}[which]
    gd, ud = g0.double().requires_grad_(True), u0.double().requires_grad_(True)
    yd = ref.textbook(gd, ud, act)
    yd.backward(dy.double())
    if which.startswith("packed"):
        layout = which.split("_")[1]
        gu = (torch.cat((g0, u0), -1) if layout == "halves" else ref.interleave(g0, u0)).requires_grad_(True)
        fused = lambda: pkg.glu_packed(gu, act=act, layout=layout)
        y = fused()
        y.backward(dy)
        assert gu.grad.shape == gu.shape
        dgate, dup = (gu.grad[:, :n], gu.grad[:, n:]) if layout == "halves" else (gu.grad[:, 0::2], gu.grad[:, 1::2])
        if layout == "interleaved":
            _eq(pkg.glu_packed(gu.detach(), act=act), y.detach(), "swiglu_oai defaults to the interleaved layout")
    else:
        g, u = g0.clone().requires_grad_(True), u0.clone().requires_grad_(True)
        fused = {"swiglu": lambda: pkg.swiglu(g, u), "geglu_tanh": lambda: pkg.geglu(g, u),
                 "geglu_none": lambda: pkg.geglu(g, u, approximate="none")}[which]
        y = fused()
        y.backward(dy)
        dgate, dup = g.grad, u.grad
    _close(y, yd)
    _close(dgate, gd.grad)
    _close(dup, ud.grad)
    with torch.no_grad():
        y2 = fused()
    assert not y2.requires_grad
    _eq(y2, y.detach(), "no_grad vs grad-enabled")


def test_autograd_takes_chunk_views_of_a_3d_projection_without_a_copy(pkg, monkeypatch):
    n = 96
    gen = torch.Generator().manual_seed(5)
    gu0 = 3 * torch.randn(2, 17, 2 * n, generator=gen).to(DEV)
    dy = torch.randn(2, 17, n, generator=gen).to(DEV)
    gu = gu0.clone().requires_grad_(True)
    calls = []
    real = pkg.activations._launch

    def spy(name, d, t, *ptrs):
        calls.append((name, int(d.rows), int(d.n), int(d.ld), ptrs))
        return real(name, d, t, *ptrs)

    monkeypatch.setattr(pkg.activations, "_launch", spy)
    gate, up = gu.chunk(2, -1)
    y = pkg.swiglu(gate, up)
    y.backward(dy)
    monkeypatch.undo()
    assert y.shape == (2, 17, n)
    base = gu.data_ptr()
    (fname, frows, fn_, fld, fptrs), (bname, brows, bn, bld, bptrs) = calls
    assert (fname, frows, fn_, fld) == ("nnop_glu", 34, n, 2 * n) and (bname, brows, bn, bld) == ("nnop_glu_bwd", 34, n, 2 * n)
    assert fptrs[1:] == (base, base + n * 4), "the forward was handed a copy, not the storage of gu"
    assert bptrs[3:] == (base, base + n * 4), "the pullback was handed a copy, not the saved views"
    gd = gu0.double().requires_grad_(True)
    a, b = gd.chunk(2, -1)
    yd = ref.textbook(a, b, "silu")
    yd.backward(dy.double())
    _close(y, yd)
    _close(gu.grad, gd.grad)
    with torch.no_grad():
        _eq(pkg.swiglu(*gu.chunk(2, -1)), y.detach(), "no_grad vs grad-enabled")
