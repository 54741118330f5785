"""GPU tests of the mixture-of-experts gate and dispatch plan (include/nnop_hip_moe.h) against tests/moe_ref.py: the header's formulas in
fp64 on the rounded inputs, selection by a lexicographic sort, the plan by a stable argsort.  Gates are the project's own and are not
widened: idx and the whole plan exact; w rtol TOL["f32"] of tests/test_softmax_gpu.py (2e-6) with atol 1e-7 (one fp32 ulp of the
largest possible weight: w is fp32 computed from exactly representable inputs); lse the same rtol with atol 2e-6 max(1, |ref|);
dlogits GTOL[dt] of that file with atol scaled by max(1, max|ref|).  What the kernels reach is recorded in profiles/moe/parity.json
(every comparison logs its ratio through util.record_error; tools/moe_parity.py keeps the worst).

Shapes are the smallest that reach every path: every register shape of the 16-byte and of the element-wise layout (E from 1 to 1024,
powers of two and 7, 60, 65, 160), one row and row counts that leave the last wave and the last workgroup ragged, a row stride above E.
Inputs are N(0, 3^2) rounded to the dtype: in bf16 several per cent of the rows then have a tie exactly at the k-th place
(tests/test_zzz_moe_host.py checks that), so the tie rule is exercised by ordinary data.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

import moe_ref as ref
from util import TORCH_DT, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ES = (1, 2, 7, 8, 32, 60, 64, 65, 128, 160, 256, 512, 1024)
KS = (1, 2, 4, 8, 16, "E")                     # "E": k = E, where E <= 16
TS = (1, 37, 257, 1030)
DTS = ("f32", "f16", "bf16")
INF, NAN = float("inf"), float("nan")


def _ks(E):
    return [k for k in KS if (k == "E" and E <= 16) or (k != "E" and k <= min(E, 16))]


def _grid():
    """Two cases per (E, dtype): one with ld = E and one with ld = E + 3, of opposite norms; k, T, the norm of the first and the use of
    dlse cycle so that every value of each occurs with every dtype (checked below)."""
    cases = []
    for (i, E), (j, dt) in itertools.product(enumerate(ES), enumerate(DTS)):
        ks = _ks(E)
        for v, pad in enumerate((0, 3)):
            n = i + j + v
            k = ks[(i + 2 * j + v) % len(ks)]
            cases.append((E, dt, E if k == "E" else k, "E" if k == "E" else k, TS[(i + j + 2 * v) % 4], E + pad, ref.NORMS[n % 2], bool((i + v) % 2)))
    return cases


GRID = _grid()
for _dt in DTS:
    _mine = [c for c in GRID if c[1] == _dt]
    assert {c[0] for c in _mine} == set(ES) and {c[3] for c in _mine} == set(KS) and {c[4] for c in _mine} == set(TS)
    assert {c[5] - c[0] for c in _mine} == {0, 3} and {c[6] for c in _mine} == set(ref.NORMS) and {c[7] for c in _mine} == {False, True}
    assert all({(c[5] - c[0], c[6]) for c in _mine if c[0] == E} in ({(0, "topk"), (3, "all")}, {(0, "all"), (3, "topk")}) for E in ES)


def _np(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _logits(x32, dt, E):
    """the fp32 numpy matrix [T, ld] on the device in dt -> (the [T, E] view the wrappers take, the whole buffer)"""
    buf = torch.tensor(x32).to(TORCH_DT[dt]).to(DEV)
    return buf[:, :E], buf


def _log(case, dt, **ratios):
    for n, r in ratios.items():
        print(f"{case} [{dt}] {n}: error / gate = {r:.4f}")
        record_error("moe", dict(name=n, case=case, dt=dt, worst_ratio=r))
    assert all(r <= 1.0 for r in ratios.values()), (case, dt, ratios)


def _forward(pkg, case, x, k, norm, dt):
    """runs the gate on the view x, judges it against the reference, returns (got, reference)"""
    got = pkg._moe_router(x, k, norm=norm)
    want = ref.router_ref(_np(x), k, norm)
    w, idx, lse = got
    T = x.shape[0]
    assert w.dtype == torch.float32 and idx.dtype == torch.int32 and lse.dtype == torch.float32
    assert w.shape == (T, k) and idx.shape == (T, k) and lse.shape == (T,)
    np.testing.assert_array_equal(idx.cpu().numpy(), want[1], err_msg=f"{case} [{dt}] idx")
    _log(case, dt, w=ref.w_ratio(_np(w), want[0]), lse=ref.lse_ratio(_np(lse), want[2]))
    return got, want


def _backward(pkg, case, x, buf, got, k, norm, dt, use_dlse, seed):
    """the pullback into a pre-filled buffer with the strides of the logits: judged against the reference, padding untouched"""
    T, E = x.shape
    rng = np.random.default_rng(seed)
    dw = torch.tensor(rng.standard_normal((T, k)).astype(np.float32)).to(DEV)
    dlse = torch.tensor(rng.standard_normal(T).astype(np.float32)).to(DEV) if use_dlse else None
    out_buf = torch.full_like(buf, 7.0)
    out = out_buf[:, :E]
    w, idx, lse = got
    assert pkg.grad_moe_router(dw, w, idx, lse, x, norm=norm, dlse=dlse, out=out) is out
    want = ref.router_grad_ref(_np(dw), _np(x), k, norm, None if dlse is None else _np(dlse))
    _log(case, dt, dlogits=ref.dl_ratio(_np(out), want, dt))
    assert (out_buf[:, E:] == 7.0).all()
    return out, dw, dlse


@pytest.mark.parametrize("E,dt,k,_kname,T,ld,norm,use_dlse", GRID,
                         ids=[f"E{c[0]}-{c[1]}-k{c[2]}-T{c[4]}-ld{c[5]}-{c[6]}-{'dlse' if c[7] else 'nodlse'}" for c in GRID])
def test_grid(pkg, E, dt, k, _kname, T, ld, norm, use_dlse):
    x, buf = _logits(ref.make_logits(E * 1000 + T + k, T, E, ld), dt, E)
    got, _ = _forward(pkg, "grid", x, k, norm, dt)
    out, dw, dlse = _backward(pkg, "grid", x, buf, got, k, norm, dt, use_dlse, E + T)
    if norm == "topk" and not use_dlse:                              # outside idx: exact zeros (+0, bitwise)
        mask = torch.ones(T, E, dtype=torch.bool, device=DEV)
        mask.scatter_(1, got[1].long(), False)
        bits = out.contiguous().view(torch.int32 if dt == "f32" else torch.int16)
        assert (bits[mask] == 0).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("E,k", [(60, 8), (128, 4), (7, 7)])
def test_tie_heavy_logits_from_four_values(pkg, dt, E, k):
    rng = np.random.default_rng(E)
    x32 = rng.choice(np.array([-1.5, 0.0, 0.25, 2.0], np.float32), size=(257, E))
    x32[5] = 0.25                                                    # an all-equal row
    x32[6, ::2] = -0.0                                               # -0 against +0
    x32[6, 1::2] = 0.0
    x, _ = _logits(x32, dt, E)
    for norm in ref.NORMS:
        (w, idx, lse), _ = _forward(pkg, "ties", x, k, norm, dt)
        assert idx[5].tolist() == list(range(k)) and idx[6].tolist() == list(range(k))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("E,k,pad", [(7, 4, 0), (60, 8, 0), (128, 8, 0), (128, 8, 3), (1024, 16, 0)])
def test_rows_with_infinities_and_nan(pkg, dt, E, k, pad):
    """-inf with fewer than k finite entries gives zero weights; a NaN, a +inf or an all -inf row gives NaN weights for that row only and
    k distinct valid indices; the rows in between are judged like any other"""
    T = 37
    x32 = ref.make_logits(E + k, T, E, E + pad)
    x32[3, :E] = -INF
    x32[3, [E - 1, 2]] = [1.5, -0.5]                                 # two finite entries, k > 2
    x32[9, E // 2] = NAN
    x32[10, [1, E - 2]] = NAN                                        # NaN against NaN: the lower index first
    x32[10, 0] = INF
    x32[17, E - 1] = INF
    x32[18, [0, E - 1]] = INF
    x32[25, :E] = -INF
    x32[30, 0] = -INF
    x, buf = _logits(x32, dt, E)
    for norm in ref.NORMS:
        (w, idx, lse), want = _forward(pkg, "special", x, k, norm, dt)
        nan_rows = sorted(set(torch.isnan(w).any(dim=1).nonzero().flatten().tolist()))
        assert nan_rows == [9, 10, 17, 18, 25] and torch.isnan(w[nan_rows]).all() and torch.isnan(lse[nan_rows]).all()
        assert idx[3, :2].tolist() == [E - 1, 2] and (w[3, 2:] == 0).all()
        assert idx[9, 0].item() == E // 2 and idx[10, :3].tolist() == [1, E - 2, 0] and idx[25].tolist() == list(range(k))
        s = idx.sort(dim=1).values
        assert (s[:, 1:] != s[:, :-1]).all() and idx.min().item() >= 0 and idx.max().item() < E


@pytest.mark.parametrize("dt,E", [("f32", 128), ("bf16", 128), ("f16", 60)])
def test_leading_dimensions_are_flattened(pkg, dt, E):
    x3 = torch.tensor(ref.make_logits(31, 6 * 7, E)).to(TORCH_DT[dt]).to(DEV).view(6, 7, E)
    w, idx, lse = pkg._moe_router(x3, 4, norm="all")
    w2, idx2, lse2 = pkg._moe_router(x3.view(42, E), 4, norm="all")
    assert w.shape == (6, 7, 4) and idx.shape == (6, 7, 4) and lse.shape == (6, 7)
    assert torch.equal(w.view(42, 4), w2) and torch.equal(idx.view(42, 4), idx2) and torch.equal(lse.view(42), lse2)
    t = x3.transpose(0, 1)                                           # not dense: the wrapper makes it so
    w3, idx3, lse3 = pkg._moe_router(t, 4, norm="all")
    assert torch.equal(w3, w.transpose(0, 1)) and torch.equal(idx3, idx.transpose(0, 1)) and torch.equal(lse3, lse.t())
    dw = torch.ones(6, 7, 4, device=DEV)
    g = pkg.grad_moe_router(dw, w, idx, lse, x3, norm="all")
    assert g.shape == x3.shape and g.dtype == x3.dtype
    assert torch.equal(g.view(42, E), pkg.grad_moe_router(dw.view(42, 4), w2, idx2, lse2, x3.view(42, E), norm="all"))
    bufs = (torch.empty_like(w), torch.empty_like(idx), torch.empty_like(lse))
    assert all(torch.equal(a, b) for a, b in zip(pkg.moe_router_into(*bufs, x3, 4, norm="all"), (w, idx, lse)))


@pytest.mark.parametrize("norm", ref.NORMS)
@pytest.mark.parametrize("dt,return_lse", [("f32", False), ("bf16", True), ("f16", False), ("f32", True)])
def test_autograd_gives_the_gradient_of_grad_moe_router(pkg, dt, return_lse, norm):
    T, E, k = 37, 60, 4
    x, _ = _logits(ref.make_logits(41, T, E), dt, E)
    x = x.contiguous()
    w0, idx0, lse0 = pkg._moe_router(x, k, norm=norm)
    rng = np.random.default_rng(7)
    dw = torch.tensor(rng.standard_normal((T, k)).astype(np.float32)).to(DEV)
    dlse = torch.tensor(rng.standard_normal(T).astype(np.float32)).to(DEV)
    leaf = x.clone().requires_grad_(True)
    out = pkg.moe_router(leaf, k, norm=norm, return_lse=return_lse)
    assert len(out) == (3 if return_lse else 2) and torch.equal(out[0], w0) and torch.equal(out[1], idx0)
    assert out[0].requires_grad and not out[1].requires_grad
    loss = (out[0] * dw).sum() + ((out[2] * dlse).sum() if return_lse else 0.0)
    loss.backward()
    want = pkg.grad_moe_router(dw, w0, idx0, lse0, x, norm=norm, dlse=dlse if return_lse else None)
    assert leaf.grad.dtype == x.dtype and torch.equal(leaf.grad, want)
    if return_lse:                                                   # the z-loss alone: only lse carries a cotangent
        leaf.grad = None
        pkg.moe_router(leaf, k, norm=norm, return_lse=True)[2].square().sum().backward()
        want = pkg.grad_moe_router(torch.zeros_like(w0), w0, idx0, lse0, x, norm=norm, dlse=2 * lse0)
        assert torch.equal(leaf.grad, want)
    with torch.no_grad():
        w1, _ = pkg.moe_router(leaf, k, norm=norm)
    assert not w1.requires_grad and torch.equal(w1, w0)


# ---- the dispatch plan ---------------------------------------------------------------------------------------------------------------
def _plan_case(pkg, idx_np, E):
    idx = torch.tensor(idx_np.astype(np.int32)).to(DEV)
    got = pkg.moe_dispatch_plan(idx, E)
    assert all(t.dtype == torch.int32 for t in got) and got[3].shape == idx.shape
    for name, g, w in zip(("counts", "offsets", "perm", "slot"), got, ref.plan_ref(idx_np, E)):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)
    return idx, got


@pytest.mark.parametrize("T,k,E", [(1, 1, 1), (37, 2, 8), (257, 4, 128), (1030, 8, 60)])
def test_plan_equals_the_stable_argsort(pkg, T, k, E):
    rng = np.random.default_rng(T)
    _plan_case(pkg, rng.integers(0, E, size=(T, k)), E)


def test_plan_of_the_gates_own_indices(pkg):
    x, _ = _logits(ref.make_logits(3, 257, 128), "bf16", 128)
    _, idx, _ = pkg._moe_router(x, 8)
    _plan_case(pkg, idx.cpu().numpy(), 128)


@pytest.mark.parametrize("T,k,E", [(257, 4, 128), (1030, 2, 1024)])
def test_plan_with_every_token_on_expert_0(pkg, T, k, E):
    _plan_case(pkg, np.zeros((T, k), np.int64), E)


@pytest.mark.parametrize("T,k,E", [(37, 2, 8), (1030, 8, 60)])
def test_plan_skips_entries_outside_the_expert_range(pkg, T, k, E):
    rng = np.random.default_rng(T + 1)
    idx = rng.integers(0, E, size=(T, k))
    idx[rng.random((T, k)) < 0.5] = -1                               # half the entries: not local
    idx[0, 0], idx[T - 1, k - 1] = E, 2 ** 31 - 1                    # ids past E are skipped as well
    _plan_case(pkg, idx, E)
    _plan_case(pkg, np.full((T, k), -1), E)                          # nothing valid at all: perm is all -1


def test_plan_with_more_chunk_histograms_than_scan_threads(pkg):
    """T = 2056, k = 8: 16448 flat ids are 257 chunks of 64, one more than the 256 threads of a column-scan workgroup, so a thread of
    that scan owns a run of two chunks and the last threads own none.  Two runs are bitwise equal; a workspace pre-filled with
    garbage gives the same result."""
    import ctypes as C
    T, k, E = 2056, 8, 60
    d = pkg._lib_moe.MoePlanDesc(tokens=T, topk=k, experts=E)
    nbytes = pkg._lib_moe.load().nnop_moe_plan_workspace_bytes(C.byref(d))
    assert nbytes == 257 * E * 4 + (-257 * E * 4) % 16
    rng = np.random.default_rng(0)
    idx_np = rng.integers(0, E, size=(T, k))
    idx_np[rng.random((T, k)) < 0.1] = -1
    idx, got = _plan_case(pkg, idx_np, E)
    again = pkg.moe_dispatch_plan(idx, E)
    ws = torch.randint(0, 256, (nbytes + 64,), dtype=torch.uint8, device=DEV)
    new = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)
    dirty = pkg.moe_dispatch_plan_into(new(E), new(E + 1), new(T * k), new(T, k), idx, E, workspace=ws)
    for a, b, c in zip(got, again, dirty):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_router_and_plan_compose_into_an_moe_layer(pkg):
    """gather by perm // k, one matmul per expert over offsets, combine by slot and w == every expert on every token, masked"""
    T, D, E, k = 257, 64, 8, 2
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(T, D, generator=g).to(DEV)
    wr = (torch.randn(D, E, generator=g) / 8).to(DEV)
    we = (torch.randn(E, D, D, generator=g) / 8).to(DEV)
    w, idx, _ = pkg._moe_router(x @ wr, k)
    counts, offsets, perm, slot = pkg.moe_dispatch_plan(idx, E)
    off = offsets.tolist()
    assert off[E] == T * k
    xs = x[(perm // k).long()]                                       # [T k, D], expert-sorted
    ys = torch.empty_like(xs)
    for e in range(E):
        ys[off[e]:off[e + 1]] = xs[off[e]:off[e + 1]] @ we[e]
    y = (ys[slot.long()] * w[..., None]).sum(dim=1)                  # [T, k, D] weighted and summed
    gate = torch.zeros(T, E, device=DEV).scatter_(1, idx.long(), w)
    dense = torch.einsum("td,edf,te->tf", x, we, gate)
    np.testing.assert_allclose(_np(y), _np(dense), rtol=1e-4, atol=1e-5)
