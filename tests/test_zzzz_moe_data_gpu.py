"""GPU tests of the mixture-of-experts permute and weighted combine (include/nnop_hip_moe_data.h) against tests/moe_data_ref.py: the
header's four formulas in fp64 on the rounded inputs.  The gates are derived there from the unit roundoffs and the contract (fp32 sums in
ascending j, one rounding on the store; dw any-order fp32) and are not widened: xs exact; y, dx, dys and dw by the formulas at the head of
that file.  What the kernels reach is recorded in profiles/moe_data/parity.json (every comparison logs error / gate through
util.record_error; tools/moe_data_parity.py keeps the worst).

Shapes are the smallest that reach every path: D = 1 (one element), 7 (odd), 8 (one 16-byte piece of a 16-bit type), 64, 520 (a ragged last
wave-load), 1030 (no multiple of the vector: the element-wise path, and the looping form of the combine pullback) and 2880 (gpt-oss: several
column chunks, the 256-lane form of the combine pullback); one token and token counts that leave the last workgroup ragged; k from 1 to
17 (more than four batches of the reduce, an odd pair count of the pullback); row strides D, D + 3 (element-wise) and D + 8 (the
strided 16-byte path).  Only -1 marks a skipped entry here: the guard against other out-of-range values is read in the code, not run.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

import moe_data_ref as ref
from util import TORCH_DT, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DS = (1, 7, 8, 64, 520, 1030, 2880)
TS = (1, 37, 257)
KS = (1, 2, 4, 8, 17)
ES = (1, 8, 60)
PADS = (0, 3, 8)
DTS = ("f32", "f16", "bf16")


def _grid():
    """Three cases per (D, dtype), one per row-stride pad; T, k, E and the share of skipped entries cycle so that every value of each
    occurs with every dtype (checked below)."""
    cases = []
    for (i, D), (j, dt) in itertools.product(enumerate(DS), enumerate(DTS)):
        for v, pad in enumerate(PADS):
            n = i + j + v
            cases.append((D, dt, pad, TS[(i + 2 * j + v) % 3], KS[(2 * i + j + v) % 5], ES[(i + j + 2 * v) % 3], (0.0, 0.3)[n % 2]))
    return cases


GRID = _grid()
for _dt in DTS:
    _mine = [c for c in GRID if c[1] == _dt]
    assert {c[0] for c in _mine} == set(DS) and {c[2] for c in _mine} == set(PADS) and {c[3] for c in _mine} == set(TS)
    assert {c[4] for c in _mine} == set(KS) and {c[5] for c in _mine} == set(ES) and {c[6] for c in _mine} == {0.0, 0.3}
    assert all({c[2] for c in _mine if c[0] == D} == set(PADS) for D in DS)


def _np(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _dev(a, dt=None):
    t = torch.tensor(np.asarray(a))
    return (t if dt is None else t.to(TORCH_DT[dt])).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _log(case, dt, **ratios):
    for n, r in ratios.items():
        print(f"{case} [{dt}] {n}: error / gate = {r:.4f}")
        record_error("moe_data", dict(name=n, case=case, dt=dt, worst_ratio=r))
    assert all(r <= 1.0 for r in ratios.values()), (case, dt, ratios)


def _out(n, D, ld, dt):
    """an output buffer [n, ld]: NaN where the call has to write, 7.0 in the padding columns -> (the [n, D] view, the buffer)"""
    buf = torch.full((n, ld), 7.0, dtype=TORCH_DT[dt], device=DEV)
    buf[:, :D] = float("nan")
    return buf[:, :D], buf


def _written(view, buf, D):
    assert not torch.isnan(view).any() and (buf[:, D:] == 7.0).all()


class Case:
    """the inputs of one shape on the device, the plan, and the four operations run into pre-filled buffers"""

    def __init__(self, pkg, seed, T, k, D, E, dt, pad=0, skip=0.0, idx=None):
        self.T, self.k, self.D, self.dt, self.S, self.ld = T, k, D, dt, T * k, D + pad
        self.idx, self.perm_np, self.slot_np = ref.make_plan(seed, T, k, E, skip, idx)
        self.perm, self.slot = _dev(self.perm_np), _dev(self.slot_np)
        self.w_np = ref.make_weights(seed + 1, T, k)
        self.w = _dev(self.w_np)
        mk = lambda s, n: _dev(ref.make_rows(seed + s, n, D, dt, self.ld), dt)[:, :D]
        self.x, self.dy, self.ys, self.dxs = mk(2, T), mk(3, T), mk(4, self.S), mk(5, self.S)

    def run(self, pkg):
        T, k, D, S, ld, dt = self.T, self.k, self.D, self.S, self.ld, self.dt
        (xs, xs_b), (dx, dx_b), (y, y_b), (dys, dys_b) = _out(S, D, ld, dt), _out(T, D, ld, dt), _out(T, D, ld, dt), _out(S, D, ld, dt)
        dw = torch.full((T, k), float("nan"), device=DEV)
        assert pkg.moe_permute_into(xs, self.x, self.perm) is xs
        assert pkg.grad_moe_permute_into(dx, self.dxs, self.slot) is dx
        assert pkg.moe_combine_into(y, self.ys, self.w, self.slot) is y
        got = pkg.grad_moe_combine_into(dys, dw, self.dy, self.ys, self.w, self.perm, self.slot)
        assert got[0] is dys and got[1] is dw
        for view, buf in ((xs, xs_b), (dx, dx_b), (y, y_b), (dys, dys_b)):
            _written(view, buf, D)
        assert not torch.isnan(dw).any()
        return xs, dx, y, dys, dw

    def judge(self, case, xs, dx, y, dys, dw):
        k, D, dt = self.k, self.D, self.dt
        x, ys, dxs, dy = _np(self.x), _np(self.ys), _np(self.dxs), _np(self.dy)
        want_y, A = ref.combine_ref(ys, self.w_np, self.slot_np)
        want_dx, Ax = ref.permute_bwd_ref(dxs, self.slot_np)
        want_dys, want_dw, B = ref.combine_bwd_ref(dy, ys, self.w_np, self.perm_np, self.slot_np)
        _log(case, dt, xs=ref.exact(_np(xs), ref.permute_ref(x, self.perm_np, k)), y=ref.y_ratio(_np(y), want_y, A, k, dt),
             dx=ref.y_ratio(_np(dx), want_dx, Ax, k, dt), dys=ref.dys_ratio(_np(dys), want_dys, dt),
             dw=ref.dw_ratio(_np(dw), want_dw, B, D))


@pytest.mark.parametrize("D,dt,pad,T,k,E,skip", GRID, ids=[f"D{c[0]}-{c[1]}-pad{c[2]}-T{c[3]}-k{c[4]}-E{c[5]}-skip{c[6]}" for c in GRID])
def test_grid(pkg, D, dt, pad, T, k, E, skip):
    c = Case(pkg, 1000 * D + 10 * T + k, T, k, D, E, dt, pad, skip)
    c.judge("grid", *c.run(pkg))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T,k,D,E,pad", [(37, 4, 64, 8, 0), (257, 2, 520, 60, 3), (37, 8, 1030, 8, 0)])
def test_skipped_entries_give_exact_zeros(pkg, dt, T, k, D, E, pad):
    """half the entries -1 (not local), token 0 with no valid slot at all; then a plan with nothing valid"""
    rng = np.random.default_rng(T + D)
    idx = rng.integers(0, E, size=(T, k))
    idx[rng.random((T, k)) < 0.5] = -1
    idx[0] = -1
    c = Case(pkg, D, T, k, D, E, dt, pad, idx=idx)
    xs, dx, y, dys, dw = c.run(pkg)
    c.judge("skipped", xs, dx, y, dys, dw)
    n = int((idx >= 0).sum())
    assert 0 < n < c.S and (c.perm_np[n:] == -1).all() and (c.slot_np[0] == -1).all()
    assert (_bits(xs[n:]) == 0).all() and (_bits(dys[n:]) == 0).all()                # the tail rows: +0, bitwise
    assert (_bits(dw)[torch.tensor(c.slot_np < 0).to(DEV)] == 0).all()
    assert (_bits(y[0]) == 0).all() and (_bits(dx[0]) == 0).all()
    c = Case(pkg, D + 1, T, k, D, E, dt, pad, idx=np.full((T, k), -1))
    for name, t in zip(("xs", "dx", "y", "dys", "dw"), c.run(pkg)):
        assert (_bits(t) == 0).all(), name


@pytest.mark.parametrize("dt", DTS)
def test_a_token_may_name_one_expert_twice(pkg, dt):
    """the hand-written plan of tests/test_zzz_moe_host.py: its last token is [2, 2]"""
    c = Case(pkg, 7, 4, 2, 8, 4, dt, idx=[[2, 0], [0, 2], [3, 0], [2, 2]])
    np.testing.assert_array_equal(c.slot_np, [[3, 0], [1, 4], [7, 2], [5, 6]])
    xs, dx, y, dys, dw = c.run(pkg)
    c.judge("duplicate", xs, dx, y, dys, dw)
    assert torch.equal(xs[5], c.x[3]) and torch.equal(xs[6], c.x[3])


@pytest.mark.parametrize("dt,T,k,D", [("f32", 37, 4, 520), ("bf16", 257, 8, 64), ("f16", 37, 2, 1030), ("bf16", 37, 17, 2880)])
def test_bitwise_properties(pkg, dt, T, k, D):
    c = Case(pkg, T + D, T, k, D, 8, dt)
    xs, dx, y, dys, dw = c.run(pkg)
    assert torch.equal(xs, c.x[(c.perm // k).long()])                # permute is a copy
    ones = torch.ones(T, k, device=DEV)
    assert torch.equal(dx, pkg._moe_combine(c.dxs, ones, c.perm, c.slot))            # permute_bwd = combine with every weight 1
    # the allocating forms equal the _into forms, and two runs are equal
    for _ in range(2):
        assert torch.equal(pkg._moe_permute(c.x, c.perm, c.slot), xs) and torch.equal(pkg.grad_moe_permute(c.dxs, c.slot), dx)
        assert torch.equal(pkg._moe_combine(c.ys, c.w, c.perm, c.slot), y)
        dys2, dw2 = pkg.grad_moe_combine(c.dy, c.ys, c.w, c.perm, c.slot)
        assert torch.equal(dys2, dys) and torch.equal(dw2, dw)
    assert pkg._moe_permute(c.x, c.perm, c.slot).shape == (T * k, D) and dw2.dtype == torch.float32 and dys2.dtype == c.ys.dtype


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_leading_dimensions_are_flattened(pkg, dt):
    B, L, k, D = 6, 7, 4, 64
    c = Case(pkg, 11, B * L, k, D, 8, dt, skip=0.3)
    xs, dx, y, dys, dw = c.run(pkg)
    x3, dy3, w3, slot3 = c.x.reshape(B, L, D), c.dy.reshape(B, L, D), c.w.view(B, L, k), c.slot.view(B, L, k)
    assert torch.equal(pkg._moe_permute(x3, c.perm, slot3), xs)
    g = pkg.grad_moe_permute(c.dxs, slot3)
    assert g.shape == (B, L, D) and torch.equal(g.view(B * L, D), dx)
    y3 = pkg._moe_combine(c.ys, w3, c.perm, slot3)
    assert y3.shape == (B, L, D) and torch.equal(y3.view(B * L, D), y)
    dys3, dw3 = pkg.grad_moe_combine(dy3, c.ys, w3, c.perm, slot3)
    assert dw3.shape == (B, L, k) and torch.equal(dys3, dys) and torch.equal(dw3.view(B * L, k), dw)
    t = x3.transpose(0, 1)                                           # not dense: the wrapper makes it so
    st = slot3.transpose(0, 1)
    assert torch.equal(pkg._moe_permute(t, c.perm, st), pkg._moe_permute(t.contiguous(), c.perm, st.contiguous()))
    assert torch.equal(pkg._moe_combine(c.ys, w3.transpose(0, 1), c.perm, st), y3.transpose(0, 1))


@pytest.mark.parametrize("dt,lead", [("f32", (37,)), ("bf16", (5, 8)), ("f16", (37,))])
def test_autograd_gives_the_gradients_of_the_grad_functions(pkg, dt, lead):
    T, k, D = int(np.prod(lead)), 4, 72
    c = Case(pkg, 21, T, k, D, 8, dt, skip=0.3)
    slot = c.slot.view(*lead, k)
    x = c.x.reshape(*lead, D).clone().requires_grad_(True)
    xs = pkg.moe_permute(x, c.perm, slot)
    assert xs.requires_grad and torch.equal(xs, pkg._moe_permute(c.x, c.perm, c.slot))
    assert [tuple(t.shape) for t in xs.grad_fn.saved_tensors] == [tuple(slot.shape)]          # slot alone
    xs.backward(c.dxs)
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    assert torch.equal(x.grad.view(T, D), pkg.grad_moe_permute(c.dxs, c.slot))
    ys = c.ys.clone().requires_grad_(True)
    w = c.w.view(*lead, k).clone().requires_grad_(True)
    y = pkg.moe_combine(ys, w, c.perm, slot)
    assert y.requires_grad and y.shape == (*lead, D) and torch.equal(y.view(T, D), pkg._moe_combine(c.ys, c.w, c.perm, c.slot))
    saved = y.grad_fn.saved_tensors
    assert [tuple(t.shape) for t in saved] == [(T * k, D), (*lead, k), (T * k,), (*lead, k)]  # ys, w, perm, slot: no [T, k, D] intermediate
    y.backward(c.dy.reshape(*lead, D))
    dys, dw = pkg.grad_moe_combine(c.dy, c.ys, c.w, c.perm, c.slot)
    assert torch.equal(ys.grad, dys) and torch.equal(w.grad.view(T, k), dw) and w.grad.dtype == torch.float32
    assert c.perm.grad is None and slot.grad is None and not c.perm.requires_grad
    # only w needs a gradient; a cotangent that is an expanded tensor
    w2 = c.w.clone().requires_grad_(True)
    pkg.moe_combine(c.ys, w2, c.perm, c.slot).sum().backward()
    _, dw1 = pkg.grad_moe_combine(torch.ones_like(c.dy), c.ys, c.w, c.perm, c.slot)
    assert torch.equal(w2.grad, dw1)
    # a None cotangent gives None gradients; under no_grad nothing is recorded or saved
    assert pkg.moe_data._MoePermute.backward(None, None) == (None, None, None)
    assert pkg.moe_data._MoeCombine.backward(None, None) == (None, None, None, None)
    with torch.no_grad():
        xs0, y0 = pkg.moe_permute(x, c.perm, slot), pkg.moe_combine(ys, w, c.perm, slot)
    assert xs0.grad_fn is None and y0.grad_fn is None and not xs0.requires_grad and not y0.requires_grad
    assert torch.equal(xs0, xs) and torch.equal(y0, y)


def test_router_plan_permute_and_combine_compose_into_an_moe_layer(pkg):
    """test_router_and_plan_compose_into_an_moe_layer (tests/test_zzz_moe_gpu.py) with the new calls: the layer equals every expert on
    every token, masked, and its gradients in x and in the router logits equal those of the same layer written with torch indexing"""
    T, D, E, k = 257, 64, 8, 2
    g = torch.Generator(device="cpu").manual_seed(0)
    x0 = torch.randn(T, D, generator=g).to(DEV)
    wr = (torch.randn(D, E, generator=g) / 8).to(DEV)
    we = (torch.randn(E, D, D, generator=g) / 8).to(DEV)
    gy = torch.randn(T, D, generator=g).to(DEV)

    def layer(fused):
        x = x0.clone().requires_grad_(True)
        logits = x @ wr
        logits.retain_grad()
        w, idx = pkg.moe_router(logits, k)
        counts, offsets, perm, slot = pkg.moe_dispatch_plan(idx, E)
        off = offsets.tolist()
        assert off[E] == T * k
        xs = pkg.moe_permute(x, perm, slot) if fused else x[(perm // k).long()]
        ys = torch.cat([xs[off[e]:off[e + 1]] @ we[e] for e in range(E)])
        y = pkg.moe_combine(ys, w, perm, slot) if fused else (ys[slot.long()] * w[..., None]).sum(dim=1)
        (y * gy).sum().backward()
        return y.detach(), x.grad, logits.grad, w.detach(), idx

    y, dx, dl, w, idx = layer(True)
    gate = torch.zeros(T, E, device=DEV).scatter_(1, idx.long(), w)
    dense = torch.einsum("td,edf,te->tf", x0, we, gate)
    np.testing.assert_allclose(_np(y), _np(dense), rtol=1e-4, atol=1e-5)
    y_t, dx_t, dl_t, _, _ = layer(False)
    np.testing.assert_allclose(_np(y), _np(y_t), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(_np(dx), _np(dx_t), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(_np(dl), _np(dl_t), rtol=1e-4, atol=1e-5)
