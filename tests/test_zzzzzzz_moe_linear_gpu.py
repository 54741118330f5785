"""GPU tests of the expert linear layers (include/nnop_hip_moe_linear.h) against tests/moe_linear_ref.py: the header's four formulas in
fp64 on the rounded inputs, in both weight layouts.  The gates are derived there and are not widened.  Every comparison logs
error / gate through util.record_error (tools/moe_linear_parity.py keeps the worst).

Shapes are the smallest at which the kernels can still go wrong.  The output tile is 128 x 128 and a reduction step is 64 (16-bit) or 32
(fp32) elements, so (K, N) run over (8, 8) (one 16-byte piece), (64, 24) (one full step), (520, 264) (several steps, three column tiles,
a ragged last one; more than one 256-column chunk of the fp32 bias gradient), (7, 5) (odd, below one piece) and (72, 1030) (no multiple of
8: the element-wise path; nine column tiles; three 512-column chunks of the 16-bit bias gradient).  The plans hit the edges of the 16-row
MFMA tiles, of the 64-row wave tiles and of the 128-row workgroup tile, leading, trailing and consecutive empty experts, E = 1, and 0, 1
or 40 rows behind the last expert; 700 rows in one expert give every row lane of the bias gradient more than one pass.  Row strides are
dim, dim + 3 (element-wise) and dim + 8 (the strided 16-byte path); the padding columns hold 7.0 on input and NaN in an output before the
call, like the rest of an output that is not accumulated into.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

import glu_ref
import moe_data_ref
import moe_linear_ref as ref
import moe_ref
from util import TORCH_DT, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNS = ((8, 8), (64, 24), (520, 264), (7, 5), (72, 1030))
PADS = (0, 3, 8)
DTS = ("f32", "f16", "bf16")
LAYOUTS = ("nk", "kn")
NAN = float("nan")
# (counts per expert, rows behind the last expert)
PLANS = (([257], 0), ([0, 129, 0], 0), ([0, 0, 65], 40), ([1, 15, 16, 17, 31, 33, 63, 64], 1), ([700, 0, 3], 0))


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
        record_error("moe_linear", dict(name=n, case=case, dt=dt, worst_ratio=r))
    assert all(r <= 1.0 for r in ratios.values()), (case, dt, ratios)


def _out(shape, ld, dt, fill=NAN, old=None):
    """an output buffer shape[:-1] + (ld,) that holds `fill` (NaN) everywhere, padding columns included; `old`: what the view holds
    instead, for a call that adds to it -> (the view, the buffer)"""
    buf = torch.full(tuple(shape[:-1]) + (ld,), fill, dtype=TORCH_DT[dt], device=DEV)
    view = buf[..., :shape[-1]]
    if old is not None:
        view.copy_(old)
    return view, buf


def _padding_kept(buf, dim, fill=NAN):
    return bool((_bits(buf[..., dim:]) == _bits(torch.full_like(buf[..., dim:], fill))).all())


def _gdts(dt):
    return (dt,) if dt == "f32" else (dt, "f32")


class Case:
    """the inputs of one shape on the device -- the same weights in both layouts -- and the four calls run into pre-filled buffers"""

    def __init__(self, seed, counts, tail, K, N, dt, pad=0, offsets=None, ints=False):
        self.off_np = ref.offsets_of(counts) if offsets is None else np.asarray(offsets, np.int32)
        self.E, self.S, self.K, self.N, self.dt, self.pad = len(counts), int(sum(counts)) + tail, K, N, dt, pad
        self.off = _dev(self.off_np)
        E, S = self.E, self.S
        if ints:
            mk = lambda s, shape: _dev(ref.make_ints(seed + s, shape), dt)
        else:
            mk = lambda s, shape: _dev(ref.make(seed + s, shape, dt, shape[-1] + pad), dt)[..., :shape[-1]]
        self.xs, self.dys, self.bias = mk(1, (S, K)), mk(2, (S, N)), mk(4, (E, N))
        w_nk = mk(3, (E, N, K))
        w_kn = torch.full((E, K, N + pad), 7.0, dtype=w_nk.dtype, device=DEV)[..., :N]
        w_kn.copy_(w_nk.transpose(1, 2))
        self.w = {"nk": w_nk, "kn": w_kn}
        self.ints = ints
        self._refs = {}

    def wshape(self, layout):
        return (self.E, self.N, self.K) if layout == "nk" else (self.E, self.K, self.N)

    def old(self, seed, shape, gdt):
        """what a gradient is added to: values of the gradient's type, of the size of the sums"""
        a = ref.make_ints(seed, shape, -3, 3) if self.ints else 4 * ref.make(seed, shape, "f32")
        return _dev(a, gdt)

    # ---- the four calls: every element in range is written, the padding keeps its NaN ----
    def fwd(self, pkg, layout, bias, fill=NAN, **over):
        ys, buf = _out((self.S, self.N), self.N + self.pad, self.dt, fill)
        b = over.get("b", self.bias) if bias else None
        assert pkg.moe_grouped_linear_into(ys, over.get("xs", self.xs), over.get("w", self.w[layout]), self.off, b, layout=layout) is ys
        assert _padding_kept(buf, self.N, fill)
        return ys

    def bwd_x(self, pkg, layout, fill=NAN, **over):
        dxs, buf = _out((self.S, self.K), self.K + self.pad, self.dt, fill)
        assert pkg.grad_moe_grouped_linear_x_into(dxs, over.get("dys", self.dys), over.get("w", self.w[layout]), self.off, layout=layout) is dxs
        assert _padding_kept(buf, self.K, fill)
        return dxs

    def bwd_w(self, pkg, layout, gdt, old=None, fill=NAN, **over):
        shape = self.wshape(layout)
        dw, buf = _out(shape, shape[-1] + self.pad, gdt, fill, old)
        assert pkg.grad_moe_grouped_linear_w_into(dw, over.get("dys", self.dys), over.get("xs", self.xs), self.off, layout=layout,
                                                  accumulate=old is not None) is dw
        assert _padding_kept(buf, shape[-1], fill)
        return dw

    def bwd_b(self, pkg, gdt, old=None, fill=NAN, **over):
        db, buf = _out((self.E, self.N), self.N + self.pad, gdt, fill, old)
        assert pkg.grad_moe_grouped_linear_b_into(db, over.get("dys", self.dys), self.off, accumulate=old is not None) is db
        assert _padding_kept(buf, self.N, fill)
        return db

    # ---- the references, each computed once ----
    def refs(self, what, layout="nk"):
        key = (what, layout if what == "dw" else "")
        if key not in self._refs:
            xs, dys, w, b = _np(self.xs), _np(self.dys), _np(self.w["nk"]), _np(self.bias)
            self._refs[key] = {"ys": lambda: ref.linear_ref(xs, w, self.off_np, b), "ys0": lambda: ref.linear_ref(xs, w, self.off_np, None),
                               "dxs": lambda: ref.bwd_x_ref(dys, w, self.off_np), "dw": lambda: ref.bwd_w_ref(dys, xs, self.off_np, layout),
                               "db": lambda: ref.bwd_b_ref(dys, self.off_np)}[what]()
        return self._refs[key]

    def empty(self):
        off = ref.clamp_offsets(self.off_np, self.S)
        return [e for e in range(self.E) if off[e + 1] <= off[e]]

    def outside(self):
        return torch.tensor(ref.rows_of(self.off_np, self.S) < 0).to(DEV)

    def ys_ratio(self, ys, bias):
        want, A, B = self.refs("ys" if bias else "ys0")
        return ref.worst(ref.fwd_ratios(_np(ys), want, A, B, self.K, self.dt))

    def dxs_ratio(self, dxs):
        want, A = self.refs("dxs")
        return ref.g.ratio(_np(dxs), want, A, self.N, self.dt)

    def grad_ratio(self, what, got, layout, gdt, old=None):
        want, A, R = self.refs(what, layout)
        o = None if old is None else _np(old)
        return ref.worst(ref.grad_ratios(_np(got), want if o is None else want + o, A, R, gdt, o))


@pytest.mark.parametrize("K,N,dt,pad,plan", GRID, ids=[f"K{c[0]}-N{c[1]}-{c[2]}-pad{c[3]}-plan{c[4]}" for c in GRID])
def test_grid(pkg, K, N, dt, pad, plan):
    """both layouts, with and without bias, the four calls, stored and accumulated, in the operands' type and in fp32"""
    counts, tail = PLANS[plan]
    c = Case(1000 * K + 10 * N + plan, counts, tail, K, N, dt, pad)
    rows, r = c.outside(), {}
    for layout in LAYOUTS:
        for bias in (False, True):
            ys = c.fwd(pkg, layout, bias)
            r[f"ys-{layout}-{'b' if bias else '0'}"] = c.ys_ratio(ys, bias)
            assert (_bits(ys)[rows] == 0).all()                                      # rows outside every expert: +0, and no bias
        dxs = c.bwd_x(pkg, layout)
        r[f"dxs-{layout}"] = c.dxs_ratio(dxs)
        assert (_bits(dxs)[rows] == 0).all()
        for gdt in _gdts(dt):
            dw = c.bwd_w(pkg, layout, gdt)
            r[f"dw-{layout}-{gdt}"] = c.grad_ratio("dw", dw, layout, gdt)
            old = c.old(7, c.wshape(layout), gdt)
            acc = c.bwd_w(pkg, layout, gdt, old)
            r[f"dw-{layout}-{gdt}-acc"] = c.grad_ratio("dw", acc, layout, gdt, old)
            for e in c.empty():
                assert (_bits(dw[e]) == 0).all() and torch.equal(_bits(acc[e]), _bits(old[e])), e
    for gdt in _gdts(dt):
        db = c.bwd_b(pkg, gdt)
        r[f"db-{gdt}"] = c.grad_ratio("db", db, "nk", gdt)
        old = c.old(8, (c.E, N), gdt)
        acc = c.bwd_b(pkg, gdt, old)
        r[f"db-{gdt}-acc"] = c.grad_ratio("db", acc, "nk", gdt, old)
        for e in c.empty():
            assert (_bits(db[e]) == 0).all() and torch.equal(_bits(acc[e]), _bits(old[e])), e
    _log("grid", dt, **r)


@pytest.mark.parametrize("dt,K,N,pad,plan", [("bf16", 520, 264, 0, 3), ("f32", 72, 1030, 3, 4), ("f16", 64, 24, 8, 2), ("bf16", 7, 5, 0, 1)])
def test_bitwise_against_the_grouped_gemm(pkg, dt, K, N, pad, plan):
    """"nk", no bias, gradients of the operands' type, no accumulation: the three products of the fifth library, bit for bit"""
    counts, tail = PLANS[plan]
    c = Case(plan, counts, tail, K, N, dt, pad)
    w = c.w["nk"]
    ys, dxs, dw = c.fwd(pkg, "nk", False), c.bwd_x(pkg, "nk"), c.bwd_w(pkg, "nk", dt)
    assert torch.equal(_bits(ys), _bits(pkg._moe_grouped_gemm(c.xs, w, c.off)))
    want_dxs, want_dw = pkg.grad_moe_grouped_gemm(c.dys, c.xs, w, c.off)
    assert torch.equal(_bits(dxs), _bits(want_dxs)) and torch.equal(_bits(dw), _bits(want_dw))


@pytest.mark.parametrize("dt,K,N,pad,plan", [("bf16", 520, 264, 0, 3), ("f32", 72, 1030, 3, 4), ("f16", 64, 24, 8, 2), ("bf16", 7, 5, 0, 1),
                                             ("f32", 8, 8, 0, 0)])
def test_bitwise_across_layouts(pkg, dt, K, N, pad, plan):
    """the same weights as [E, K, N]: ys and dxs are those of [E, N, K] bit for bit (the LDS images and the MFMA order are the same);
    dw of the one layout is the transpose of the other's within the gate, and whether bit for bit is logged"""
    counts, tail = PLANS[plan]
    c = Case(plan, counts, tail, K, N, dt, pad)
    assert torch.equal(c.w["kn"], c.w["nk"].transpose(1, 2))
    for bias in (False, True):
        assert torch.equal(_bits(c.fwd(pkg, "kn", bias)), _bits(c.fwd(pkg, "nk", bias))), bias
    assert torch.equal(_bits(c.bwd_x(pkg, "kn")), _bits(c.bwd_x(pkg, "nk")))
    dw_nk, dw_kn = c.bwd_w(pkg, "nk", dt), c.bwd_w(pkg, "kn", dt)
    same = torch.equal(_bits(dw_kn), _bits(dw_nk.transpose(1, 2)))
    print(f"across-layouts [{dt}] K={K} N={N}: dw_kn == dw_nk^T bit for bit: {same}")
    record_error("moe_linear", dict(name="dw_kn==dw_nk^T", case="across-layouts", dt=dt, bitwise=same))
    _log("across-layouts", dt, dw_kn=c.grad_ratio("dw", dw_kn, "kn", dt))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,N,pad", [(64, 24, 0), (40, 64, 8), (7, 5, 0), (24, 64, 3)])
def test_exact_integer_data(pkg, dt, K, N, pad):
    """integers in [-2, 2] (old: [-3, 3]), at most 64 rows per expert and K, N <= 64: every sum is an integer of magnitude <= 261, exact in
    fp32, and the one rounding to a 16-bit type is the reference's too, so the four calls equal the reference bit for bit, in both
    layouts, with the bias, in fp32 beside 16-bit operands and accumulated onto integers"""
    c = Case(K + N, [64, 0, 17, 33, 1, 63], 2, K, N, dt, pad, ints=True)
    eq = lambda got, want, gdt, name: (np.abs(want).max() <= 261 and torch.equal(_bits(got), _bits(_dev(want + 0.0, gdt)))) or pytest.fail(name)
    for layout in LAYOUTS:
        eq(c.fwd(pkg, layout, True), c.refs("ys")[0], dt, f"ys {layout}")
        eq(c.bwd_x(pkg, layout), c.refs("dxs")[0], dt, f"dxs {layout}")
        for gdt in _gdts(dt):
            eq(c.bwd_w(pkg, layout, gdt), c.refs("dw", layout)[0], gdt, f"dw {layout} {gdt}")
            old = c.old(9, c.wshape(layout), gdt)
            eq(c.bwd_w(pkg, layout, gdt, old), c.refs("dw", layout)[0] + _np(old), gdt, f"dw {layout} {gdt} accumulated")
    for gdt in _gdts(dt):
        eq(c.bwd_b(pkg, gdt), c.refs("db")[0], gdt, f"db {gdt}")
        old = c.old(10, (c.E, N), gdt)
        eq(c.bwd_b(pkg, gdt, old), c.refs("db")[0] + _np(old), gdt, f"db {gdt} accumulated")
    assert c.bias.any() and not torch.equal(c.bias[0], c.bias[2]) and not torch.equal(c.w["nk"][0], c.w["nk"][2])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_micro_batches_accumulate_into_fp32(pkg, layout):
    """bf16 operands, fp32 dw and db: the second micro-batch is added to the first; the result is inside the gate of the fp64 sum of both
    (R, A: those of the two batches together, `old`: the first batch's share).  An expert without rows in the second batch keeps the
    bits it had, a NaN pattern included; without the flag a NaN-filled gradient is overwritten."""
    K, N, dt = 72, 40, "bf16"
    a, b = Case(1, [33, 65, 17, 0], 0, K, N, dt), Case(2, [129, 0, 1, 0], 3, K, N, dt)
    dw = a.bwd_w(pkg, layout, "f32")
    db = a.bwd_b(pkg, "f32")
    pattern = torch.tensor([0x7fc01234, 0x7f800001, -1, 5], dtype=torch.int32, device=DEV).view(torch.float32)
    dw[3].view(-1)[:4], db[3][:4] = pattern, pattern                          # expert 3 has no rows in either batch
    first_w, first_b = dw.clone(), db.clone()
    assert pkg.grad_moe_grouped_linear_w_into(dw, b.dys, b.xs, b.off, layout=layout, accumulate=True) is dw
    assert pkg.grad_moe_grouped_linear_b_into(db, b.dys, b.off, accumulate=True) is db
    (wa, Aa, Ra), (wb, Ab, Rb) = a.refs("dw", layout), b.refs("dw", layout)
    (ba, Ba, Sa), (bb, Bb, Sb) = a.refs("db"), b.refs("db")
    live = [0, 1, 2]
    _log(f"micro-batches-{layout}", dt,
         dw=ref.worst(ref.grad_ratios(_np(dw)[live], (wa + wb)[live], (Aa + Ab)[live], (Ra + Rb)[live], "f32", wa[live])),
         db=ref.worst(ref.grad_ratios(_np(db)[live], (ba + bb)[live], (Ba + Bb)[live], (Sa + Sb)[live], "f32", ba[live])))
    for e in (1, 3):                                                          # no rows in the second batch: the bits stay
        assert torch.equal(_bits(dw[e]), _bits(first_w[e])) and torch.equal(_bits(db[e]), _bits(first_b[e])), e
    assert not torch.equal(_bits(dw[0]), _bits(first_w[0])) and not torch.equal(_bits(db[2]), _bits(first_b[2]))
    # without the flag: what the buffers held, NaN included, is gone
    dw.fill_(NAN), db.fill_(NAN)
    pkg.grad_moe_grouped_linear_w_into(dw, b.dys, b.xs, b.off, layout=layout)
    pkg.grad_moe_grouped_linear_b_into(db, b.dys, b.off)
    assert not torch.isnan(dw).any() and not torch.isnan(db).any() and (_bits(dw[3]) == 0).all() and (_bits(db[1]) == 0).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,N,pad", [(40, 72, 0), (72, 40, 3)])
def test_neighbour_isolation(pkg, dt, K, N, pad, layout):
    """the rows, the weights and the bias of expert e + 1 set to NaN leave everything of expert e as it was, bit for bit; expert e ends in
    the middle of a tile (17, 65, 129 rows)"""
    c = Case(K, [17, 65, 129, 5], 0, K, N, dt, pad)
    gdt = _gdts(dt)[-1]
    clean = (c.fwd(pkg, layout, True), c.bwd_x(pkg, layout), c.bwd_w(pkg, layout, gdt), c.bwd_b(pkg, gdt))
    for e in range(3):
        lo, hi, nxt = (int(c.off_np[i]) for i in (e, e + 1, e + 2))
        xs, dys, w, bias = c.xs.clone(), c.dys.clone(), c.w[layout].clone(), c.bias.clone()
        xs[hi:nxt], dys[hi:nxt], w[e + 1], bias[e + 1] = NAN, NAN, NAN, NAN
        ys, dxs = c.fwd(pkg, layout, True, xs=xs, w=w, b=bias), c.bwd_x(pkg, layout, dys=dys, w=w)
        dw, db = c.bwd_w(pkg, layout, gdt, dys=dys, xs=xs), c.bwd_b(pkg, gdt, dys=dys)
        assert torch.equal(_bits(ys[lo:hi]), _bits(clean[0][lo:hi])) and torch.equal(_bits(dxs[lo:hi]), _bits(clean[1][lo:hi])), e
        assert torch.equal(_bits(dw[e]), _bits(clean[2][e])) and torch.equal(_bits(db[e]), _bits(clean[3][e])), e
        assert torch.isnan(ys[hi:nxt]).all() and torch.isnan(dw[e + 1]).all() and torch.isnan(db[e + 1]).all()    # the NaNs did arrive


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("offsets", [[-7, 20, 90, 155], [-(2 ** 31), -1, 149, 2 ** 31 - 1], [3, 20, 150, 150]])
def test_out_of_range_offsets_are_clamped(pkg, dt, offsets):
    """entries below 0 and above S: the result is the reference's with the clamped ranges, and a guard band of NaN rows on either side
    of every output buffer is untouched"""
    S, E, K, N, G = 150, 3, 40, 72, 130
    c = Case(11, [50] * E, 0, K, N, dt, offsets=offsets)
    assert c.S == S
    T = TORCH_DT[dt]
    full = lambda *s: torch.full(s, NAN, dtype=T, device=DEV)
    ys_b, dxs_b, dw_b, db_b = full(G + S + G, N), full(G + S + G, K), full(E + 2, K, N), full(E + 2, N)
    guard = [_bits(b).clone() for b in (ys_b, dxs_b, dw_b, db_b)]
    ys, dxs, dw, db = ys_b[G:G + S], dxs_b[G:G + S], dw_b[1:E + 1], db_b[1:E + 1]
    pkg.moe_grouped_linear_into(ys, c.xs, c.w["kn"], c.off, c.bias, layout="kn")
    pkg.grad_moe_grouped_linear_x_into(dxs, c.dys, c.w["kn"], c.off, layout="kn")
    pkg.grad_moe_grouped_linear_w_into(dw, c.dys, c.xs, c.off, layout="kn")
    pkg.grad_moe_grouped_linear_b_into(db, c.dys, c.off)
    _log("clamped", dt, ys=c.ys_ratio(ys, True), dxs=c.dxs_ratio(dxs), dw=c.grad_ratio("dw", dw, "kn", dt), db=c.grad_ratio("db", db, "nk", dt))
    for b, g, (lo, hi) in zip((ys_b, dxs_b, dw_b, db_b), guard, ((G, G + S), (G, G + S), (1, E + 1), (1, E + 1))):
        now = _bits(b)
        assert torch.equal(now[:lo], g[:lo]) and torch.equal(now[hi:], g[hi:])
    assert not any(torch.isnan(t).any() for t in (ys, dxs, dw, db))
    rows = c.outside()
    assert (_bits(ys)[rows] == 0).all() and (_bits(dxs)[rows] == 0).all()


@pytest.mark.parametrize("dt,K,N,plan", [("bf16", 520, 264, 3), ("f32", 72, 1030, 4), ("f16", 64, 24, 2)])
def test_bitwise_reproducibility(pkg, dt, K, N, plan):
    """two runs into differently pre-filled buffers are equal, and the allocating forms equal the _into forms"""
    counts, tail = PLANS[plan]
    c = Case(plan, counts, tail, K, N, dt)
    gdt = _gdts(dt)[-1]
    for layout in LAYOUTS:
        run = lambda fill: (c.fwd(pkg, layout, True, fill), c.bwd_x(pkg, layout, fill), c.bwd_w(pkg, layout, gdt, None, fill),
                            c.bwd_b(pkg, gdt, None, fill))
        first = run(NAN)
        for fill in (NAN, 3.0):
            for a, b in zip(run(fill), first):
                assert torch.equal(_bits(a), _bits(b)), (layout, fill)
        w = c.w[layout]
        assert torch.equal(_bits(pkg._moe_grouped_linear(c.xs, w, c.off, c.bias, layout=layout)), _bits(first[0]))
        dxs, dw, db = pkg.grad_moe_grouped_linear(c.dys, c.xs, w, c.off, layout=layout)
        assert torch.equal(_bits(dxs), _bits(first[1])) and dw.shape == w.shape and dw.dtype == w.dtype and db.shape == (c.E, N)
        old_w, old_b = c.old(3, c.wshape(layout), gdt), c.old(4, (c.E, N), gdt)
        once = (c.bwd_w(pkg, layout, gdt, old_w), c.bwd_b(pkg, gdt, old_b))
        again = pkg.grad_moe_grouped_linear(c.dys, c.xs, w, c.off, layout=layout, needs=(False, True, True),
                                            out=(None, old_w.clone(), old_b.clone()), accumulate=True)
        assert again[0] is None and torch.equal(_bits(again[1]), _bits(once[0])) and torch.equal(_bits(again[2]), _bits(once[1]))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTS)
def test_autograd_gives_the_gradients_of_the_grad_functions(pkg, dt, layout):
    counts, tail = PLANS[3]
    c = Case(21, counts, tail, 72, 40, dt)
    w0 = c.w[layout]
    want = pkg.grad_moe_grouped_linear(c.dys, c.xs, w0, c.off, layout=layout)
    xs, w, bias = (t.clone().requires_grad_(True) for t in (c.xs, w0, c.bias))
    ys = pkg.moe_grouped_linear(xs, w, c.off, bias, layout=layout)
    assert ys.requires_grad and torch.equal(ys, pkg._moe_grouped_linear(c.xs, w0, c.off, c.bias, layout=layout))
    assert [tuple(t.shape) for t in ys.grad_fn.saved_tensors] == [(c.S, 72), tuple(w0.shape), (c.E + 1,)]         # xs, w, offsets: no bias
    ys.backward(c.dys)
    for got, exp, like in zip((xs.grad, w.grad, bias.grad), want, (xs, w, bias)):
        assert torch.equal(_bits(got), _bits(exp)) and got.dtype == like.dtype and got.shape == like.shape
    # only what asks for a gradient is launched
    calls = []
    G = pkg.moe_linear
    real = {n: getattr(G, f"grad_moe_grouped_linear_{n}_into") for n in "xwb"}
    for n in "xwb":
        setattr(G, f"grad_moe_grouped_linear_{n}_into", lambda *a, _n=n, **k: (calls.append(_n), real[_n](*a, **k))[1])
    try:
        b1 = c.bias.clone().requires_grad_(True)
        pkg.moe_grouped_linear(c.xs, w0, c.off, b1, layout=layout).backward(c.dys)
        assert calls == ["b"] and torch.equal(_bits(b1.grad), _bits(want[2]))
        x1 = c.xs.clone().requires_grad_(True)
        pkg.moe_grouped_linear(x1, w0, c.off, c.bias, layout=layout).backward(c.dys)              # a bias without requires_grad: no bwd_b
        assert calls == ["b", "x"] and torch.equal(_bits(x1.grad), _bits(want[0])) and c.bias.grad is None
        w1 = w0.clone().requires_grad_(True)
        pkg.moe_grouped_linear(c.xs, w1, c.off, layout=layout).backward(c.dys)                    # no bias at all
        assert calls == ["b", "x", "w"] and torch.equal(_bits(w1.grad), _bits(want[1]))
        assert pkg.grad_moe_grouped_linear(c.dys, c.xs, w0, c.off, layout=layout, needs=(False, False, False)) == (None, None, None)
        only = pkg.grad_moe_grouped_linear(c.dys, c.xs, w0, c.off, layout=layout, needs=(False, True, False))
        assert calls == ["b", "x", "w", "w"] and only[0] is None and only[2] is None and torch.equal(_bits(only[1]), _bits(want[1]))
    finally:
        for n in "xwb":
            setattr(G, f"grad_moe_grouped_linear_{n}_into", real[n])
    assert G._MoeGroupedLinear.backward(None, None) == (None,) * 5
    with torch.no_grad():
        y0 = pkg.moe_grouped_linear(xs, w, c.off, bias, layout=layout)
    assert y0.grad_fn is None and not y0.requires_grad and torch.equal(y0, ys)


# ---- the gpt-oss layer ---------------------------------------------------------------------------------------------------------------
T_, E_, K_, H_, I_ = 97, 8, 2, 64, 40


def _layer_inputs(dt):
    """the expert tensors in the checkpoint's form: gate_up_proj [E, H, 2I] + [E, 2I], down_proj [E, I, H] + [E, H]"""
    mk = lambda s, shape, scale=1.0: _dev(ref.make(s, shape, dt, scale=scale), dt)
    return dict(x=mk(1, (T_, H_)), wr=mk(2, (H_, E_), 0.3), gate_up_proj=mk(3, (E_, H_, 2 * I_), 0.15), gate_up_bias=mk(6, (E_, 2 * I_), 0.5),
                down_proj=mk(4, (E_, I_, H_), 0.15), down_bias=mk(7, (E_, H_), 0.5), dy=mk(5, (T_, H_)))


def _layer(pkg, p, x, logits):
    """router -> plan -> permute -> linear -> glu -> linear -> combine; every intermediate is returned"""
    w, idx, lse = pkg.moe_router(logits, K_, return_lse=True)
    counts, offsets, perm, slot = pkg.moe_dispatch_plan(idx, E_)
    xs = pkg.moe_permute(x, perm, slot)
    h = pkg.moe_grouped_linear(xs, p["gate_up_proj"], offsets, p["gate_up_bias"], layout="kn")
    a = pkg.glu_packed(h, layout="interleaved", act="swiglu_oai")
    ys = pkg.moe_grouped_linear(a, p["down_proj"], offsets, p["down_bias"], layout="kn")
    y = pkg.moe_combine(ys, w, perm, slot)
    return dict(w=w, idx=idx, lse=lse, counts=counts, offsets=offsets, perm=perm, slot=slot, xs=xs, h=h, a=a, ys=ys, y=y)


def _expert_linear(rows, W, b, off):
    """rows[s] @ W[e] + b[e] for the rows of expert e, zeros behind the last expert: the formula as the model's code states it, fp64"""
    out = np.zeros((rows.shape[0], W.shape[2]))
    for e in range(W.shape[0]):
        out[off[e]:off[e + 1]] = rows[off[e]:off[e + 1]] @ W[e] + b[e]
    return out


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_the_gpt_oss_layer(pkg, dt):
    """the expert MLP of gpt-oss through the project's kernels with the checkpoint's four expert tensors as they are, forward and
    backward.  Each stage is judged by its own derived gate against the fp64 formula, written out here, on the device's output of the
    stage before (an end-to-end bound would have to be calibrated; the stages' bounds are derived)."""
    p = _layer_inputs(dt)
    x = p["x"].clone().requires_grad_(True)
    logits = (p["x"] @ p["wr"]).requires_grad_(True)
    names = ("gate_up_proj", "gate_up_bias", "down_proj", "down_bias")
    q = dict(p, **{n: p[n].clone().requires_grad_(True) for n in names})
    r = _layer(pkg, q, x, logits)
    r["y"].backward(p["dy"])
    torch.cuda.synchronize()
    d = {n: t.detach() for n, t in r.items()}
    off, slot, perm = (d[n].cpu().numpy() for n in ("offsets", "slot", "perm"))
    np.testing.assert_array_equal(d["idx"].cpu().numpy(), moe_ref.router_ref(_np(logits), K_, "topk")[1])
    np.testing.assert_array_equal(off, moe_ref.plan_ref(d["idx"].cpu().numpy(), E_)[1])
    W1, b1, W2, b2 = (_np(p[n]) for n in names)
    # forward: h = xs @ gate_up_proj[e] + bias, a = swiglu_oai(h even, h odd), ys = a @ down_proj[e] + bias, y = sum_j w_j ys[slot_j]
    want_h, want_ys = _expert_linear(_np(d["xs"]), W1, b1, off), _expert_linear(_np(d["a"]), W2, b2, off)
    _, Ah, Bh = ref.linear_ref(_np(d["xs"]), W1, off, b1, "kn")
    _, Ays, Bys = ref.linear_ref(_np(d["a"]), W2, off, b2, "kn")
    want_y, Ay = moe_data_ref.combine_ref(_np(d["ys"]), _np(d["w"]), slot)
    _log("gpt-oss", dt, xs=moe_data_ref.exact(_np(d["xs"]), moe_data_ref.permute_ref(_np(p["x"]), perm, K_)),
         h=ref.worst(ref.fwd_ratios(_np(d["h"]), want_h, Ah, Bh, H_, dt)),
         a=glu_ref.gate_ok(d["a"], glu_ref.glu_ref(d["h"][:, 0::2], d["h"][:, 1::2], "swiglu_oai"), dt),
         ys=ref.worst(ref.fwd_ratios(_np(d["ys"]), want_ys, Ays, Bys, I_, dt)), y=moe_data_ref.y_ratio(_np(d["y"]), want_y, Ay, K_, dt))
    n = int(off[-1])
    assert (_bits(d["h"][n:]) == 0).all() and (_bits(d["ys"][n:]) == 0).all()
    # backward: the gradients of .backward() are those of the hand-chained grad_* calls, bit for bit ...
    dys, dgate = pkg.grad_moe_combine(p["dy"], d["ys"], d["w"], d["perm"], d["slot"])
    da, dW2, db2 = pkg.grad_moe_grouped_linear(dys, d["a"], p["down_proj"], d["offsets"], layout="kn")
    dh = pkg.grad_glu_packed(da, d["h"], act="swiglu_oai", layout="interleaved")
    dxs, dW1, db1 = pkg.grad_moe_grouped_linear(dh, d["xs"], p["gate_up_proj"], d["offsets"], layout="kn")
    dx = pkg.grad_moe_permute(dxs, d["slot"])
    dl = pkg.grad_moe_router(dgate, d["w"], d["idx"], d["lse"], logits.detach())
    for name, got, want in (("x", x.grad, dx), ("logits", logits.grad, dl), ("gate_up_proj", q[names[0]].grad, dW1),
                            ("gate_up_bias", q[names[1]].grad, db1), ("down_proj", q[names[2]].grad, dW2), ("down_bias", q[names[3]].grad, db2)):
        assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), name
    # ... and each pullback of the two projections is the formula's on the device's cotangent: da = dys @ W2[e]^T,
    # dW2[e] = a[e]^T dys[e], db2[e] = sum_s dys[s], and the same one stage down
    g2, g1 = _np(dys), _np(dh)
    ratios = {}
    for tag, gy, xin, W, dxg, dWg, dbg in (("2", g2, _np(d["a"]), W2, da, dW2, db2), ("1", g1, _np(d["xs"]), W1, dxs, dW1, db1)):
        want_dx = np.zeros_like(xin)
        want_dW, want_db = np.zeros_like(W), np.zeros((E_, W.shape[2]))
        for e in range(E_):
            lo, hi = off[e], off[e + 1]
            want_dx[lo:hi], want_dW[e], want_db[e] = gy[lo:hi] @ W[e].T, xin[lo:hi].T @ gy[lo:hi], gy[lo:hi].sum(0)
        _, Ax = ref.bwd_x_ref(gy, W, off, "kn")
        _, AW, RW = ref.bwd_w_ref(gy, xin, off, "kn")
        _, Ab, Rb = ref.bwd_b_ref(gy, off)
        ratios.update({f"dx{tag}": ref.g.ratio(_np(dxg), want_dx, Ax, W.shape[2], dt),
                       f"dW{tag}": ref.worst(ref.grad_ratios(_np(dWg), want_dW, AW, RW, dt)),
                       f"db{tag}": ref.worst(ref.grad_ratios(_np(dbg), want_db, Ab, Rb, dt))})
    want_dh = glu_ref.interleave(*glu_ref.glu_grads_ref(da, d["h"][:, 0::2], d["h"][:, 1::2], "swiglu_oai"))
    _log("gpt-oss-bwd", dt, dh=glu_ref.gate_ok(dh, want_dh, dt), **ratios)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_the_layer_is_captured_in_a_graph(pkg, dt):
    """the same layer forward, so the forward call twice, and the three pullback calls of the second projection (the weight and bias
    gradients accumulated into fp32), captured on one stream and replayed once: the replay equals the eager run bit for bit"""
    p = _layer_inputs(dt)
    logits = p["x"] @ p["wr"]
    dys = _dev(ref.make(9, (T_ * K_, H_), dt), dt)
    main_w, main_b = _dev(ref.make(10, (E_, I_, H_), "f32")), _dev(ref.make(11, (E_, H_), "f32"))

    def run():
        r = _layer(pkg, p, p["x"], logits)
        dw, db = main_w.clone(), main_b.clone()
        r["da"], r["dw"], r["db"] = pkg.grad_moe_grouped_linear(dys, r["a"], p["down_proj"], r["offsets"], layout="kn", out=(None, dw, db),
                                                                accumulate=True)
        return r

    with torch.no_grad():
        eager = run()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()                                                                # warm-up on the capture's side of things
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = run()
        for t in captured.values():
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
    for name in ("offsets", "xs", "h", "a", "ys", "y", "da", "dw", "db"):
        assert torch.equal(_bits(captured[name]), _bits(eager[name])), name
