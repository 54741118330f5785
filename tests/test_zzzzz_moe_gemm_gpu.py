"""GPU tests of the grouped expert GEMM (include/nnop_hip_moe_gemm.h) against tests/moe_gemm_ref.py: the header's three formulas in fp64
on the rounded inputs.  The gate is derived there (u |ref| + (R + 2) 2^-23 A + floor, the any-order bound of an R-term fp32 sum and one
rounding on the store) and is not widened.  Every comparison logs error / gate through util.record_error (tools/moe_gemm_parity.py keeps
the worst).

Shapes are the smallest at which the kernel can still go wrong.  The output tile is 128 x 128 and a reduction step is 64 (16-bit) or 32
(fp32) elements, so (K, N) run over (8, 8) (one 16-byte piece), (64, 24) (one full step), (40, 72) (a ragged step), (520, 264) (several
steps, three column tiles, a ragged last one), (1030, 8) and (72, 1030) (no multiple of 8: the element-wise path; nine column tiles) and
(7, 5) (odd, below one piece).  Row counts per expert are written out, from {0, 1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 257},
so that the edges of the 16-row MFMA tiles, of the 64-row wave tiles and of the 128-row workgroup tile are hit on both sides: leading,
trailing and consecutive empty experts, E = 1, every row in the last expert, and 0, 1 or 40 rows behind the last expert.  Row strides are
dim, dim + 3 (element-wise) and dim + 8 (the strided 16-byte path); the padding columns hold 7.0 on input and NaN, like the rest of the
buffer, in an output before the call.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

import glu_ref
import moe_data_ref
import moe_gemm_ref as ref
import moe_ref
from util import TORCH_DT, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNS = ((8, 8), (64, 24), (40, 72), (520, 264), (1030, 8), (7, 5), (72, 1030))
PADS = (0, 3, 8)
DTS = ("f32", "f16", "bf16")
NAN = float("nan")


def _sixty():
    c = [0] * 60
    for i, n in enumerate((0, 1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129)):
        c[5 * i] = n
    c[58] = c[59] = 1
    return c


# (counts per expert, rows behind the last expert)
PLANS = (([257], 0), ([17], 1), ([0, 129, 0], 0), ([0, 0, 65], 40), ([1, 15, 16, 17, 31, 33, 63, 64], 1),
         ([65, 0, 0, 127, 128, 129, 0, 1], 0), (_sixty(), 40))
assert {len(p[0]) for p in PLANS} == {1, 3, 8, 60} and {p[1] for p in PLANS} == {0, 1, 40}
assert {n for p in PLANS for n in p[0]} == {0, 1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 257}
assert max(sum(p[0]) + p[1] for p in PLANS) <= 700


def _grid():
    """Three cases per ((K, N), dtype), one per row-stride pad; the plans cycle so that every plan occurs with every dtype and every pad"""
    cases = []
    for (i, kn), (j, dt) in itertools.product(enumerate(KNS), enumerate(DTS)):
        for v, pad in enumerate(PADS):
            cases.append((kn[0], kn[1], dt, pad, (i + 2 * j + 3 * v) % len(PLANS)))
    return cases


GRID = _grid()
for _dt in DTS:
    _mine = [c for c in GRID if c[2] == _dt]
    assert {c[4] for c in _mine} == set(range(len(PLANS))) and {(c[0], c[1]) for c in _mine} == set(KNS)
for _pad in PADS:
    assert {c[4] for c in GRID if c[3] == _pad} == set(range(len(PLANS)))


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
        record_error("moe_gemm", dict(name=n, case=case, dt=dt, worst_ratio=r))
    assert all(r <= 1.0 for r in ratios.values()), (case, dt, ratios)


def _out(shape, ld, dt, fill=NAN):
    """an output buffer shape[:-1] + (ld,) that holds `fill` (NaN) everywhere, padding columns included -> (the view, the buffer)"""
    buf = torch.full(tuple(shape[:-1]) + (ld,), fill, dtype=TORCH_DT[dt], device=DEV)
    return buf[..., :shape[-1]], buf


class Case:
    """the inputs of one shape on the device and the three products run into pre-filled buffers"""

    def __init__(self, seed, counts, tail, K, N, dt, pad=0, offsets=None, ints=False):
        self.off_np = ref.offsets_of(counts) if offsets is None else np.asarray(offsets, np.int32)
        self.E, self.S, self.K, self.N, self.dt, self.pad = len(counts), int(sum(counts)) + tail, K, N, dt, pad
        self.off = _dev(self.off_np)
        if ints:
            mk = lambda s, shape: _dev(ref.make_ints(seed + s, shape), dt)
        else:
            mk = lambda s, shape: _dev(ref.make(seed + s, shape, dt, shape[-1] + pad), dt)[..., :shape[-1]]
        self.xs, self.dys, self.w = mk(1, (self.S, K)), mk(2, (self.S, N)), mk(3, (self.E, N, K))

    def run(self, pkg, fill=NAN, xs=None, dys=None, w=None):
        S, E, K, N, dt, pad = self.S, self.E, self.K, self.N, self.dt, self.pad
        xs, dys, w = (self.xs if xs is None else xs), (self.dys if dys is None else dys), (self.w if w is None else w)
        (ys, ys_b), (dxs, dxs_b), (dw, dw_b) = _out((S, N), N + pad, dt, fill), _out((S, K), K + pad, dt, fill), _out((E, N, K), K + pad, dt, fill)
        assert pkg.moe_grouped_gemm_into(ys, xs, w, self.off) is ys
        assert pkg.grad_moe_grouped_gemm_x_into(dxs, dys, w, self.off) is dxs
        assert pkg.grad_moe_grouped_gemm_w_into(dw, dys, xs, self.off) is dw
        for view, buf, dim in ((ys, ys_b, N), (dxs, dxs_b, K), (dw, dw_b, K)):
            assert not torch.isnan(view).any()                                       # every element in range is written
            assert (_bits(buf[..., dim:]) == _bits(torch.full_like(buf[..., dim:], fill))).all()     # the padding: still NaN, bit for bit
        return ys, dxs, dw

    def refs(self):
        xs, dys, w = _np(self.xs), _np(self.dys), _np(self.w)
        return ref.gemm_ref(xs, w, self.off_np), ref.bwd_x_ref(dys, w, self.off_np), ref.bwd_w_ref(dys, xs, self.off_np)

    def judge(self, case, ys, dxs, dw):
        (want_y, Ay), (want_dx, Ax), (want_dw, Aw, Rw) = self.refs()
        _log(case, self.dt, ys=ref.ratio(_np(ys), want_y, Ay, self.K, self.dt), dxs=ref.ratio(_np(dxs), want_dx, Ax, self.N, self.dt),
             dw=ref.ratio(_np(dw), want_dw, Aw, Rw, self.dt))
        off = ref.clamp_offsets(self.off_np, self.S)
        outside = np.ones(self.S, bool)
        for _, lo, hi in ref.ranges(self.off_np, self.S):
            outside[lo:hi] = False
        rows = torch.tensor(outside).to(DEV)
        assert (_bits(ys)[rows] == 0).all() and (_bits(dxs)[rows] == 0).all()         # rows outside every expert: +0, the sign bit clear
        for e in range(self.E):
            if off[e + 1] <= off[e]:
                assert (_bits(dw[e]) == 0).all(), e                                  # an expert without rows: +0 everywhere


@pytest.mark.parametrize("K,N,dt,pad,plan", GRID, ids=[f"K{c[0]}-N{c[1]}-{c[2]}-pad{c[3]}-plan{c[4]}" for c in GRID])
def test_grid(pkg, K, N, dt, pad, plan):
    counts, tail = PLANS[plan]
    c = Case(1000 * K + 10 * N + plan, counts, tail, K, N, dt, pad)
    c.judge("grid", *c.run(pkg))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,N,skip", [(64, 24, 0.3), (520, 264, 0.1), (7, 5, 0.5)])
def test_offsets_of_the_dispatch_plan(pkg, dt, K, N, skip):
    """offsets as moe_dispatch_plan writes them from random expert ids with a share of -1"""
    T, k, E = 67, 4, 8
    idx, _, _ = moe_data_ref.make_plan(K + N, T, k, E, skip)
    counts, offsets, perm, slot = pkg.moe_dispatch_plan(_dev(idx), E)
    c = Case(K, counts.tolist(), T * k - int(counts.sum()), K, N, dt, offsets=_np(offsets).astype(np.int32))
    assert c.S == T * k and c.off_np[E] < c.S
    c.off = offsets                                                              # the plan's own tensor
    c.judge("plan", *c.run(pkg))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,N,pad", [(64, 24, 0), (40, 64, 8), (7, 5, 0), (24, 64, 3)])
def test_exact_integer_data(pkg, dt, K, N, pad):
    """integers in [-2, 2], at most 64 rows per expert and K, N <= 64: every result is an integer of magnitude <= 256, exact in every
    type, so the three products equal the reference bit for bit.  The weights are not symmetric and differ between the experts."""
    c = Case(K + N, [64, 0, 17, 33, 1, 63], 2, K, N, dt, pad, ints=True)
    ys, dxs, dw = c.run(pkg)
    (want_y, _), (want_dx, _), (want_dw, _, _) = c.refs()
    for name, got, want in (("ys", ys, want_y), ("dxs", dxs, want_dx), ("dw", dw, want_dw)):
        assert np.abs(want).max() <= 256
        assert torch.equal(_bits(got), _bits(_dev(want + 0.0, dt))), name
    assert not torch.equal(c.w[0], c.w[2]) and (K != N or not torch.equal(c.w[0], c.w[0].t()))


@pytest.mark.parametrize("dt", DTS)
def test_one_hot_rows_copy_weight_columns(pkg, dt):
    """xs[s] = the unit vector of column s % K: ys[s] is column s % K of the expert's weights, readable as it stands"""
    K, N, counts = 40, 24, [17, 0, 65, 33]
    c = Case(5, counts, 3, K, N, dt)
    cols = torch.arange(c.S, device=DEV) % K
    xs = torch.zeros(c.S, K, dtype=TORCH_DT[dt], device=DEV)
    xs[torch.arange(c.S, device=DEV), cols] = 1.0
    ys = pkg._moe_grouped_gemm(xs, c.w, c.off)
    for e, lo, hi in ref.ranges(c.off_np, c.S):
        assert torch.equal(ys[lo:hi], c.w[e][:, cols[lo:hi]].t()), e
    assert (_bits(ys[sum(counts):]) == 0).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,N,pad", [(40, 72, 0), (72, 40, 3)])
def test_neighbour_isolation(pkg, dt, K, N, pad):
    """the rows and the weights of expert e + 1 set to NaN leave everything of expert e as it was, bit for bit; expert e ends in the middle
    of a tile (17, 65, 129 rows)"""
    counts = [17, 65, 129, 5]
    c = Case(K, counts, 0, K, N, dt, pad)
    clean = c.run(pkg)
    for e in range(3):
        lo, hi, nxt = int(c.off_np[e]), int(c.off_np[e + 1]), int(c.off_np[e + 2])
        xs, dys, w = c.xs.clone(), c.dys.clone(), c.w.clone()
        xs[hi:nxt], dys[hi:nxt], w[e + 1] = NAN, NAN, NAN
        S, E = c.S, c.E
        ys, dxs, dw = torch.empty(S, N, dtype=xs.dtype, device=DEV), torch.empty(S, K, dtype=xs.dtype, device=DEV), torch.empty_like(c.w)
        pkg.moe_grouped_gemm_into(ys, xs, w, c.off)
        pkg.grad_moe_grouped_gemm_x_into(dxs, dys, w, c.off)
        pkg.grad_moe_grouped_gemm_w_into(dw, dys, xs, c.off)
        assert torch.equal(_bits(ys[lo:hi]), _bits(clean[0][lo:hi])), e
        assert torch.equal(_bits(dxs[lo:hi]), _bits(clean[1][lo:hi])), e
        assert torch.equal(_bits(dw[e]), _bits(clean[2][e])), e
        assert torch.isnan(ys[hi:nxt]).all() and torch.isnan(dw[e + 1]).all()     # the NaNs did arrive where they belong


@pytest.mark.parametrize("dt", DTS)
def test_zero_rows_in_zero_rows_out(pkg, dt):
    """xs from moe_permute under a plan with skipped entries: the tail rows of ys are +0, and they stay +0 where the tail of xs is
    overwritten with NaN, because tail rows are never read"""
    T, k, E, K, N = 67, 2, 8, 72, 40
    idx, _, _ = moe_data_ref.make_plan(3, T, k, E, 0.3)
    counts, offsets, perm, slot = pkg.moe_dispatch_plan(_dev(idx), E)
    n = int(counts.sum())
    assert 0 < n < T * k
    x = _dev(ref.make(1, (T, K), dt), dt)
    w = _dev(ref.make(2, (E, N, K), dt), dt)
    xs = pkg._moe_permute(x, perm, slot)
    assert (_bits(xs[n:]) == 0).all()
    ys = pkg._moe_grouped_gemm(xs, w, offsets)
    assert (_bits(ys[n:]) == 0).all() and not torch.isnan(ys).any()
    xs[n:] = NAN
    ys2 = pkg._moe_grouped_gemm(xs, w, offsets)
    assert torch.equal(_bits(ys2), _bits(ys))
    dys = _dev(ref.make(4, (T * k, N), dt), dt)
    dys[n:] = NAN
    dxs, dw = pkg.grad_moe_grouped_gemm(dys, xs, w, offsets)
    assert (_bits(dxs[n:]) == 0).all() and not torch.isnan(dxs).any() and not torch.isnan(dw).any()


@pytest.mark.parametrize("dt,K,N,plan", [("bf16", 520, 264, 5), ("f32", 72, 1030, 4), ("f16", 1030, 8, 6), ("bf16", 64, 24, 3)])
def test_bitwise_reproducibility(pkg, dt, K, N, plan):
    """two runs are equal, the result does not depend on what the output buffer held, and the allocating forms equal the _into forms"""
    counts, tail = PLANS[plan]
    c = Case(plan, counts, tail, K, N, dt)
    first = c.run(pkg, fill=NAN)
    for fill in (NAN, 3.0):
        for a, b in zip(c.run(pkg, fill=fill), first):
            assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(pkg._moe_grouped_gemm(c.xs, c.w, c.off)), _bits(first[0]))
    dxs, dw = pkg.grad_moe_grouped_gemm(c.dys, c.xs, c.w, c.off)
    assert torch.equal(_bits(dxs), _bits(first[1])) and torch.equal(_bits(dw), _bits(first[2]))
    assert dxs.shape == (c.S, K) and dw.shape == (c.E, N, K) and dw.dtype == c.w.dtype
    # rows that are not dense: the wrapper makes them so
    t = c.xs.t().contiguous().t()
    assert not t.is_contiguous() and torch.equal(_bits(pkg._moe_grouped_gemm(t, c.w, c.off)), _bits(first[0]))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("offsets", [[-7, 20, 90, 155], [-(2 ** 31), -1, 149, 2 ** 31 - 1], [3, 20, 150, 150]])
def test_out_of_range_offsets_are_clamped(pkg, dt, offsets):
    """entries below 0 and above S: the result is the reference's with the clamped ranges, and a guard band of NaN rows on either side
    of every output buffer is untouched"""
    S, E, K, N, G = 150, 3, 40, 72, 130
    c = Case(11, [50] * E, 0, K, N, dt, offsets=offsets)
    assert c.S == S
    T = TORCH_DT[dt]
    ys_b, dxs_b = torch.full((G + S + G, N), NAN, dtype=T, device=DEV), torch.full((G + S + G, K), NAN, dtype=T, device=DEV)
    dw_b = torch.full((E + 2, N, K), NAN, dtype=T, device=DEV)
    guard = [_bits(b).clone() for b in (ys_b, dxs_b, dw_b)]
    ys, dxs, dw = ys_b[G:G + S], dxs_b[G:G + S], dw_b[1:E + 1]
    pkg.moe_grouped_gemm_into(ys, c.xs, c.w, c.off)
    pkg.grad_moe_grouped_gemm_x_into(dxs, c.dys, c.w, c.off)
    pkg.grad_moe_grouped_gemm_w_into(dw, c.dys, c.xs, c.off)
    c.judge("clamped", ys, dxs, dw)
    for b, g, (lo, hi) in zip((ys_b, dxs_b, dw_b), guard, ((G, G + S), (G, G + S), (1, E + 1))):
        now = _bits(b)
        assert torch.equal(now[:lo], g[:lo]) and torch.equal(now[hi:], g[hi:])
    assert not torch.isnan(ys).any() and not torch.isnan(dxs).any() and not torch.isnan(dw).any()


@pytest.mark.parametrize("dt", DTS)
def test_autograd_gives_the_gradients_of_the_grad_functions(pkg, dt):
    counts, tail = PLANS[4]
    c = Case(21, counts, tail, 72, 40, dt)
    want_dxs, want_dw = pkg.grad_moe_grouped_gemm(c.dys, c.xs, c.w, c.off)
    xs, w = c.xs.clone().requires_grad_(True), c.w.clone().requires_grad_(True)
    ys = pkg.moe_grouped_gemm(xs, w, c.off)
    assert ys.requires_grad and torch.equal(ys, pkg._moe_grouped_gemm(c.xs, c.w, c.off))
    assert [tuple(t.shape) for t in ys.grad_fn.saved_tensors] == [(c.S, 72), (c.E, 40, 72), (c.E + 1,)]        # xs, w, offsets
    ys.backward(c.dys)
    assert torch.equal(_bits(xs.grad), _bits(want_dxs)) and torch.equal(_bits(w.grad), _bits(want_dw))
    assert xs.grad.dtype == xs.dtype and w.grad.dtype == w.dtype and c.off.grad is None
    # only one of the two asks for a gradient: the other product is not launched
    calls = []
    G = pkg.moe_gemm
    real_x, real_w = G.grad_moe_grouped_gemm_x_into, G.grad_moe_grouped_gemm_w_into
    G.grad_moe_grouped_gemm_x_into = lambda *a: (calls.append("x"), real_x(*a))[1]
    G.grad_moe_grouped_gemm_w_into = lambda *a: (calls.append("w"), real_w(*a))[1]
    try:
        xs1 = c.xs.clone().requires_grad_(True)
        pkg.moe_grouped_gemm(xs1, c.w, c.off).backward(c.dys)
        assert calls == ["x"] and torch.equal(_bits(xs1.grad), _bits(want_dxs))
        w1 = c.w.clone().requires_grad_(True)
        pkg.moe_grouped_gemm(c.xs, w1, c.off).backward(c.dys)
        assert calls == ["x", "w"] and torch.equal(_bits(w1.grad), _bits(want_dw)) and c.xs.grad is None
        assert pkg.grad_moe_grouped_gemm(c.dys, c.xs, c.w, c.off, needs=(False, False)) == (None, None) and calls == ["x", "w"]
        only_x = pkg.grad_moe_grouped_gemm(c.dys, c.xs, c.w, c.off, needs=(True, False))
        only_w = pkg.grad_moe_grouped_gemm(c.dys, c.xs, c.w, c.off, needs=(False, True))
        assert calls == ["x", "w", "x", "w"] and only_x[1] is None and only_w[0] is None
        assert torch.equal(_bits(only_x[0]), _bits(want_dxs)) and torch.equal(_bits(only_w[1]), _bits(want_dw))
    finally:
        G.grad_moe_grouped_gemm_x_into, G.grad_moe_grouped_gemm_w_into = real_x, real_w
    # caller-owned buffers through `out`; a None cotangent gives None gradients; under no_grad nothing is recorded
    bx, bw = torch.empty_like(c.xs), torch.empty_like(c.w)
    got = pkg.grad_moe_grouped_gemm(c.dys, c.xs, c.w, c.off, out=(bx, bw))
    assert got[0] is bx and got[1] is bw and torch.equal(_bits(bx), _bits(want_dxs)) and torch.equal(_bits(bw), _bits(want_dw))
    assert G._MoeGroupedGemm.backward(None, None) == (None, None, None)
    with torch.no_grad():
        y0 = pkg.moe_grouped_gemm(xs, w, c.off)
    assert y0.grad_fn is None and not y0.requires_grad and torch.equal(y0, ys)


def test_weight_offsets_past_two_to_the_31(pkg):
    """E N ld_w > 2^31 elements: the last rows of the second expert's weights lie behind element 2^31 of w and of dw.  Only the last 8
    columns of dys are non-zero, so the references need those 8 weight rows alone (a zero adds nothing to a sum or to its gate)."""
    E, N, K, dt = 2, 32776, 32768, "bf16"
    assert (E - 1) * N * K + (N - 8) * K > 2 ** 31
    off_np = ref.offsets_of([8, 16])
    S, lo = 24, 8
    off = _dev(off_np)
    g = torch.Generator(device=DEV).manual_seed(5)
    w = torch.empty(E, N, K, dtype=torch.bfloat16, device=DEV).normal_(generator=g)
    xs = torch.empty(S, K, dtype=torch.bfloat16, device=DEV).normal_(generator=g)
    dys = torch.zeros(S, N, dtype=torch.bfloat16, device=DEV)
    dys[:, N - 8:].normal_(generator=g)
    ys = pkg._moe_grouped_gemm(xs, w, off)
    dxs, dw = pkg.grad_moe_grouped_gemm(dys, xs, w, off)
    torch.cuda.synchronize()
    x1, g1, w1 = _np(xs[lo:]), _np(dys[lo:, N - 8:]), _np(w[1, N - 8:])
    _log("past-2^31", dt, ys=ref.ratio(_np(ys[lo:, N - 8:]), x1 @ w1.T, np.abs(x1) @ np.abs(w1).T, K, dt),
         dxs=ref.ratio(_np(dxs[lo:]), g1 @ w1, np.abs(g1) @ np.abs(w1), N, dt),
         dw=ref.ratio(_np(dw[1, N - 8:]), g1.T @ x1, np.abs(g1).T @ np.abs(x1), 16, dt))
    assert (_bits(dw[1, :8]) == 0).all()                                             # rows of dw that only zeros of dys reach
    del w, dw
    torch.cuda.empty_cache()


# ---- the layer ------------------------------------------------------------------------------------------------------------------------
T_, E_, K_, H_, I_ = 67, 8, 2, 72, 40


def _layer_inputs(dt):
    mk = lambda s, shape, scale=1.0: _dev(ref.make(s, shape, dt, scale=scale), dt)
    return dict(x=mk(1, (T_, H_)), wr=mk(2, (H_, E_), 0.3), w1=mk(3, (E_, 2 * I_, H_), 0.15), w2=mk(4, (E_, H_, I_), 0.15), dy=mk(5, (T_, H_)))


def _layer(pkg, p, act, x, logits):
    """router -> plan -> permute -> GEMM -> glu -> GEMM -> combine; every intermediate is returned"""
    w, idx, lse = pkg.moe_router(logits, K_, return_lse=True)
    counts, offsets, perm, slot = pkg.moe_dispatch_plan(idx, E_)
    xs = pkg.moe_permute(x, perm, slot)
    h = pkg.moe_grouped_gemm(xs, p["w1"], offsets)
    a = pkg.glu_packed(h, act)
    ys = pkg.moe_grouped_gemm(a, p["w2"], offsets)
    y = pkg.moe_combine(ys, w, perm, slot)
    return dict(w=w, idx=idx, lse=lse, counts=counts, offsets=offsets, perm=perm, slot=slot, xs=xs, h=h, a=a, ys=ys, y=y)


@pytest.mark.parametrize("act", ["swiglu_oai", "silu"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_the_layer_composes(pkg, dt, act):
    """the whole expert MLP through the project's kernels, forward and backward, with offsets never leaving the device; each stage is
    judged by its own gate against its own reference on the device's output of the stage before"""
    p = _layer_inputs(dt)
    x = p["x"].clone().requires_grad_(True)
    logits = (p["x"] @ p["wr"]).requires_grad_(True)
    w1, w2 = p["w1"].clone().requires_grad_(True), p["w2"].clone().requires_grad_(True)
    q = dict(p, w1=w1, w2=w2)
    r = _layer(pkg, q, act, x, logits)
    r["y"].backward(p["dy"])
    torch.cuda.synchronize()
    # the forward, stage by stage
    want_w, want_idx, _ = moe_ref.router_ref(_np(logits), K_, "topk")
    idx = r["idx"].cpu().numpy()
    np.testing.assert_array_equal(idx, want_idx)
    _, want_off, want_perm, want_slot = moe_ref.plan_ref(idx, E_)
    off, perm, slot = (r[n].cpu().numpy() for n in ("offsets", "perm", "slot"))
    np.testing.assert_array_equal(off, want_off), np.testing.assert_array_equal(perm, want_perm), np.testing.assert_array_equal(slot, want_slot)
    want_h, Ah = ref.gemm_ref(_np(r["xs"]), _np(p["w1"]), off)
    want_ys, Ays = ref.gemm_ref(_np(r["a"]), _np(p["w2"]), off)
    want_y, Ay = moe_data_ref.combine_ref(_np(r["ys"]), _np(r["w"]), slot)
    layout = "interleaved" if act == "swiglu_oai" else "halves"
    hd = r["h"].detach()
    gate, up = (hd[:, 0::2], hd[:, 1::2]) if layout == "interleaved" else (hd[:, :I_], hd[:, I_:])
    _log(f"layer-{act}", dt, w=moe_ref.w_ratio(_np(r["w"]), want_w), xs=moe_data_ref.exact(_np(r["xs"]), moe_data_ref.permute_ref(_np(p["x"]), perm, K_)),
         h=ref.ratio(_np(r["h"]), want_h, Ah, H_, dt), a=glu_ref.gate_ok(r["a"], glu_ref.glu_ref(gate, up, act), dt),
         ys=ref.ratio(_np(r["ys"]), want_ys, Ays, I_, dt), y=moe_data_ref.y_ratio(_np(r["y"]), want_y, Ay, K_, dt))
    # the gradients of .backward() are those of the hand-chained grad_* calls, bit for bit
    d = {n: t.detach() for n, t in r.items()}
    dys, dgate = pkg.grad_moe_combine(p["dy"], d["ys"], d["w"], d["perm"], d["slot"])
    da, dw2 = pkg.grad_moe_grouped_gemm(dys, d["a"], p["w2"], d["offsets"])
    dh = pkg.grad_glu_packed(da, d["h"], act=act)
    dxs, dw1 = pkg.grad_moe_grouped_gemm(dh, d["xs"], p["w1"], d["offsets"])
    dx = pkg.grad_moe_permute(dxs, d["slot"])
    dl = pkg.grad_moe_router(dgate, d["w"], d["idx"], d["lse"], logits.detach())
    for name, got, want in (("x", x.grad, dx), ("w1", w1.grad, dw1), ("w2", w2.grad, dw2), ("logits", logits.grad, dl)):
        assert torch.equal(_bits(got), _bits(want)), name
    # and the pullbacks of the two GEMMs pass their gates on the device's cotangents
    (want_da, Aa), (want_dw2, Aw2, Rw2) = ref.bwd_x_ref(_np(dys), _np(p["w2"]), off), ref.bwd_w_ref(_np(dys), _np(d["a"]), off)
    (want_dxs, Ax), (want_dw1, Aw1, Rw1) = ref.bwd_x_ref(_np(dh), _np(p["w1"]), off), ref.bwd_w_ref(_np(dh), _np(d["xs"]), off)
    _log(f"layer-{act}-bwd", dt, da=ref.ratio(_np(da), want_da, Aa, H_, dt), dw2=ref.ratio(_np(dw2), want_dw2, Aw2, Rw2, dt),
         dxs=ref.ratio(_np(dxs), want_dxs, Ax, 2 * I_, dt), dw1=ref.ratio(_np(dw1), want_dw1, Aw1, Rw1, dt))


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_the_layer_is_captured_in_a_graph(pkg, dt):
    """the same composition under torch.cuda.graph capture and one replay, with the default hardware queues: the replay's output equals
    the eager output bit for bit"""
    p = _layer_inputs(dt)
    logits = p["x"] @ p["wr"]
    with torch.no_grad():
        eager = _layer(pkg, p, "swiglu_oai", p["x"], logits)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _layer(pkg, p, "swiglu_oai", p["x"], logits)                         # warm-up on the capture's side of things
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = _layer(pkg, p, "swiglu_oai", p["x"], logits)
        for t in captured.values():
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
    for name in ("offsets", "xs", "h", "a", "ys", "y"):
        assert torch.equal(_bits(captured[name]), _bits(eager[name])), name
