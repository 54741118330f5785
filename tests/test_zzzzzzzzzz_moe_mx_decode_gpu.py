"""GPU tests of the weight-streaming MXFP4 expert layer (include/nnop_hip_moe_mx_decode.h).  Results are judged against the fp64 formulas
of tests/moe_linear_ref.py on tests/mx_ref.py's dequantised values under the derived gate of that file, which depends on no summation
order and passes through neither the project's GEMM nor its dequantiser; what the header promises bit for bit (rows outside the experts,
padding, batch invariance, selection, reproducibility) is compared bit for bit.  Every ratio is logged through util.record_error.

Shapes are the smallest at which this kernel can still go wrong.  A block is 32 values, a reduction step 128 (4 blocks, one per k group
of the MFMA), the ring holds 2 steps, an MFMA is 16 rows x 16 columns, a wave owns 64 columns and a workgroup 256: (K, N) = (32, 8) is one
block, three k groups idle; (64, 24) half a step; (96, 136) a ragged step, three waves; (544, 264) 17 blocks -- five steps, a ragged
last one, an odd count for the ring -- and two workgroups per expert; (160, 5) an odd N: the element-wise store; (2880, 48) the K of
gpt-oss: 90 blocks, so the ring wraps and ends on a ragged step.  The plans hold experts of 0 rows, of 1, of 16 and 17 (a row group and
one over), of 31, 33 (one over a pass), 63, 64, 65 and 700 rows (many passes), rows behind the last expert, and a first expert without
rows.  Row strides are dim, dim + 3 and dim + 8; the padding columns hold 7.0 on input and NaN in an output before the call.  Weights are
random codes with scale bytes uniform in 119 ... 131 (|w| <= 96), so sums stay far from the overflow of float16.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

import moe_linear_ref as ref
import mx_ref
from util import TORCH_DT, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNS = ((32, 8), (64, 24), (96, 136), (544, 264), (160, 5), (2880, 48))
PADS = (0, 3, 8)
DTS = ("f16", "bf16")
NAN = float("nan")
# (counts per expert, rows behind the last expert)
PLANS = (([1], 0), ([0, 2, 0], 0), ([3, 0, 1, 2], 2), ([16], 0), ([17], 0), ([1, 15, 16, 17, 31, 33, 63, 64], 1), ([0, 0, 65], 40),
         ([700, 0, 3], 0))


def _grid():
    """One case per ((K, N), dtype, pad); the plans cycle so that every plan occurs with every dtype and with every pad"""
    cases = []
    for (i, kn), (j, dt), (v, pad) in itertools.product(enumerate(KNS), enumerate(DTS), enumerate(PADS)):
        cases.append((kn[0], kn[1], dt, pad, (i + 4 * j + 3 * v) % len(PLANS)))
    return cases


GRID = _grid()
assert {(c[0], c[1], c[2], c[3]) for c in GRID} == set((k, n, dt, pad) for (k, n), dt, pad in itertools.product(KNS, DTS, PADS))
for _dt in DTS:
    assert {c[4] for c in GRID if c[2] == _dt} == set(range(len(PLANS)))
for _pad in PADS:
    assert {c[4] for c in GRID if c[3] == _pad} == set(range(len(PLANS)))


def _np(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _dev(a, dt=None):
    t = torch.tensor(np.asarray(a))
    return (t if dt is None else t.to(TORCH_DT[dt])).to(DEV)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _log(case, dt, **ratios):
    for n, r in ratios.items():
        print(f"{case} [{dt}] {n}: error / gate = {r:.4f}")
        record_error("moe_mx_decode", dict(name=n, case=case, dt=dt, worst_ratio=r))
    assert all(r <= 1.0 for r in ratios.values()), (case, dt, ratios)


class Case:
    """the inputs of one shape on the device, the packed weights, and the decode forward run into a NaN-filled padded buffer"""

    def __init__(self, pkg, seed, counts, tail, K, N, dt, pad=0, offsets=None, scales=None, x_scale=1.0):
        self.pkg = pkg
        self.off_np = ref.offsets_of(counts) if offsets is None else np.asarray(offsets, np.int32)
        self.E, self.S, self.K, self.N, self.dt, self.pad = len(counts), int(sum(counts)) + tail, K, N, dt, pad
        self.off = _dev(self.off_np)
        mk = lambda s, shape, scale=1.0: _dev(ref.make(seed + s, shape, dt, shape[-1] + pad, scale), dt)[..., :shape[-1]]
        self.xs, self.dys, self.bias = mk(1, (self.S, K), x_scale), mk(2, (self.S, N)), mk(4, (self.E, N))
        self.blocks_np, self.scales_np = mx_ref.random_packed(seed + 3, (self.E, N, K))
        if scales is not None:
            scales(self.scales_np)
        self.set_weights()
        self._refs = {}

    def set_weights(self):
        self.blocks, self.scales = _dev(self.blocks_np), _dev(self.scales_np)

    def fwd(self, bias, xs=None, off=None):
        """every element in range is written, the padding keeps its NaN"""
        buf = torch.full((self.S, self.N + self.pad), NAN, dtype=TORCH_DT[self.dt], device=DEV)
        ys = buf[:, :self.N]
        got = self.pkg.moe_decode_linear_mxfp4_into(ys, self.xs if xs is None else xs, self.blocks, self.scales,
                                                    self.off if off is None else off, self.bias if bias else None)
        assert got is ys
        assert bool((_bits(buf[:, self.N:]) == _bits(torch.full_like(buf[:, self.N:], NAN))).all())
        return ys

    def ratio(self, ys, bias):
        """against the fp64 formula on mx_ref's weights, computed once per (case, bias)"""
        if bias not in self._refs:
            w = mx_ref.dequant(self.blocks_np, self.scales_np, self.dt)
            self._refs[bias] = ref.linear_ref(_np(self.xs), w, self.off_np, _np(self.bias) if bias else None)
        want, A, B = self._refs[bias]
        return ref.worst(ref.fwd_ratios(_np(ys), want, A, B, self.K, self.dt))

    def outside(self):
        return torch.tensor(ref.rows_of(self.off_np, self.S) < 0).to(DEV)


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,dt,pad,plan", GRID, ids=[f"K{c[0]}-N{c[1]}-{c[2]}-pad{c[3]}-plan{c[4]}" for c in GRID])
def test_grid(pkg, K, N, dt, pad, plan):
    """with and without bias: inside the derived gate of the fp64 formula on mx_ref's weights, rows outside every expert all bits zero,
    padding kept"""
    counts, tail = PLANS[plan]
    c = Case(pkg, 1000 * K + 10 * N + plan, counts, tail, K, N, dt, pad)
    rows, r = c.outside(), {}
    for bias in (False, True):
        ys = c.fwd(bias)
        r[f"ys-{'b' if bias else '0'}"] = c.ratio(ys, bias)
        assert (_bits(ys)[rows] == 0).all()
    _log("grid", dt, **r)


# ---- batch invariance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_a_rows_bits_do_not_depend_on_the_plan(pkg, dt):
    """the same x rows reach the same experts in two plans over the same weights: at other positions of their expert's range, in another
    row group and another pass (so beside another number of accumulator groups), with other neighbours, another S and other rows in
    front of and behind the experts.  Their ys bits are equal, with and without bias"""
    K, N = 544, 72
    a = Case(pkg, 41, [5, 20, 3], 0, K, N, dt)
    b = Case(pkg, 43, [40, 37, 0], 2, K, N, dt)
    b.blocks_np, b.scales_np, b.bias = a.blocks_np, a.scales_np, a.bias
    b.set_weights()
    xs = b.xs.clone()
    # expert 0: its 5 rows of plan a (one accumulator group) become slots 3 ... 7 of 40 rows (a pass of 32 with two groups); expert 1: the
    # first 5 of its 20 rows (two groups) become slots 32 ... 36 of 37 rows (the second pass, one group), the other 15 slots 9 ... 23
    moves = ((0, 5, 3), (5, 10, 72), (10, 25, 49))
    for lo, hi, to in moves:
        xs[to:to + hi - lo] = a.xs[lo:hi]
    for bias in (False, True):
        ya, yb = a.fwd(bias), b.fwd(bias, xs=xs)
        assert torch.isfinite(ya).all()
        for lo, hi, to in moves:
            assert _same_bits(ya[lo:hi], yb[to:to + hi - lo]), (bias, lo)
        assert not _same_bits(yb[:5], ya[:5])                        # other rows did give other results
    _log("invariance", dt, ys=a.ratio(a.fwd(True), True))


# ---- selection --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_other_experts_and_rows_behind_the_plan_never_enter(pkg, dt):
    """every block of expert 1 carries the scale byte 255 and the rows behind offsets[E] hold NaN: the rows of experts 0 and 2 are finite
    and what they are without either, bit for bit; the NaN expert's rows are NaN, the rows behind the plan +0"""
    c = Case(pkg, 5, [17, 33, 30], 20, 96, 136, dt)
    clean = c.fwd(True)
    c.scales_np[1] = 255
    c.set_weights()
    xs = c.xs.clone()
    xs[80:] = NAN
    ys = c.fwd(True, xs=xs)
    for lo, hi in ((0, 17), (50, 80)):
        assert torch.isfinite(ys[lo:hi]).all() and _same_bits(ys[lo:hi], clean[lo:hi])
    assert torch.isnan(ys[17:50]).all() and (_bits(ys[80:]) == 0).all()


@pytest.mark.parametrize("dt", DTS)
def test_one_block_reaches_exactly_what_depends_on_it(pkg, dt):
    """scales[1][n0][b0] = 255: column n0 of expert 1's rows is NaN and everything else keeps its bits; then the scale byte 254 with all
    16 bytes of that block 0x77 (every weight +Inf): the same column is not finite, everything else keeps its bits"""
    K, N, n0, b0 = 160, 24, 13, 3
    c = Case(pkg, 6, [40, 70, 19], 0, K, N, dt)
    clean = c.fwd(False)
    hit = torch.zeros_like(clean, dtype=torch.bool)
    hit[40:110, n0] = True
    c.scales_np[1, n0, b0] = 255
    c.set_weights()
    ys = c.fwd(False)
    assert torch.isnan(ys[hit]).all() and torch.equal(_bits(ys)[~hit], _bits(clean)[~hit])
    c.scales_np[1, n0, b0], c.blocks_np[1, n0, b0] = 254, 0x77
    c.set_weights()
    ys = c.fwd(False)
    assert not torch.isfinite(ys[hit]).any() and torch.equal(_bits(ys)[~hit], _bits(clean)[~hit])


@pytest.mark.parametrize("dt", DTS)
def test_small_scales_stay_inside_the_gate(pkg, dt):
    """scale bytes 0, 1, 2 (weights that are subnormal or zero in the 16-bit types), 113, 114 (the edge of float16's normal range) and
    140, 141 (its top: at 141 the magnitudes 4 and 6 are Inf in float16, as the format defines and the reference has it) among the
    ordinary ones.  The rows are scaled by 2^-5 so that the finite sums stay far inside float16; bytes at which an fp32 partial sum
    overflows are not here: what such a sum gives depends on the order"""
    def edges(s):
        flat = s.reshape(-1)
        flat[::3] = np.resize(np.array([0, 1, 2, 113, 114, 140, 141], np.uint8), flat[::3].size)
    c = Case(pkg, 7, [33, 16, 5], 3, 96, 40, dt, scales=edges, x_scale=2.0 ** -5)
    assert {0, 1, 2, 113, 114, 140, 141} <= set(c.scales_np.reshape(-1).tolist())
    w = mx_ref.dequant(c.blocks_np, c.scales_np, dt)
    assert (w == 0).any() and (dt != "f16" or (np.abs(w[w != 0]).min() < 2.0 ** -14))
    _log("small-scales", dt, ys=c.ratio(c.fwd(True), True), ys0=c.ratio(c.fwd(False), False))


# ---- offsets ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [[-7, 20, 90, 155], [-(2 ** 31), -1, 149, 2 ** 31 - 1], [3, 20, 150, 150], [120, 60, 140, 10]])
def test_out_of_range_offsets_touch_nothing_outside(pkg, offsets):
    """entries below 0, above S, and decreasing: a guard band of NaN rows on either side of ys is untouched; with non-decreasing entries
    the result is inside the gate for the clamped ranges, with +0 outside them"""
    S, E, K, N, G, dt = 150, 3, 96, 136, 130, "bf16"
    c = Case(pkg, 11, [50] * E, 0, K, N, dt, offsets=offsets)
    band = torch.full((G + S + G, N), NAN, dtype=TORCH_DT[dt], device=DEV)
    guard = _bits(band).clone()
    ys = band[G:G + S]
    pkg.moe_decode_linear_mxfp4_into(ys, c.xs, c.blocks, c.scales, c.off, c.bias)
    torch.cuda.synchronize()
    now = _bits(band)
    assert torch.equal(now[:G], guard[:G]) and torch.equal(now[G + S:], guard[G + S:])
    if offsets == sorted(offsets):
        _log("clamped", dt, ys=c.ratio(ys, True))
        assert (_bits(ys)[c.outside()] == 0).all()


# ---- the tile path, autograd, reproducibility, capture ----------------------------------------------------------------------------------
def test_integer_data_agrees_with_the_tile_path_exactly(pkg):
    """codes 0, +-1, +-2 at the scale byte 127 are those integers and every sum is exact in either order: the two forwards are equal"""
    g = torch.Generator(device=DEV).manual_seed(2)
    off = torch.tensor([0, 33, 33, 97, 150], dtype=torch.int32, device=DEV)
    code_of = torch.tensor([12, 10, 0, 2, 4], dtype=torch.uint8, device=DEV)                 # -2, -1, 0, 1, 2
    wi = torch.randint(-2, 3, (4, 40, 32), generator=g, device=DEV)
    codes = code_of[wi + 2]
    blocks = (codes[..., 0::2] | (codes[..., 1::2] << 4)).reshape(4, 40, 1, 16).contiguous()
    scales = torch.full((4, 40, 1), 127, dtype=torch.uint8, device=DEV)
    for dt in (torch.bfloat16, torch.float16):
        xq, bias = (torch.randint(-2, 3, s, generator=g, device=DEV).to(dt) for s in ((160, 32), (4, 40)))
        for b in (None, bias):
            got, tile = pkg.moe_decode_linear_mxfp4(xq, blocks, scales, off, b), pkg.moe_grouped_linear_mxfp4(xq, blocks, scales, off, b)
            assert torch.equal(got, tile)
            for e, (lo, hi) in enumerate(((0, 33), (33, 33), (33, 97), (97, 150))):
                want = xq[lo:hi].float() @ wi[e].float().t() + (0 if b is None else b[e].float())
                assert torch.equal(got[lo:hi].float(), want)
            assert (_bits(got[150:]) == 0).all()


@pytest.mark.parametrize("dt", DTS)
def test_autograd_gives_the_gradients_of_the_into_calls(pkg, dt):
    counts, tail = PLANS[5]
    c = Case(pkg, 21, counts, tail, 96, 40, dt)
    want_dxs, want_db = torch.empty_like(c.xs), torch.empty_like(c.bias)
    pkg.grad_moe_grouped_linear_mxfp4_x_into(want_dxs, c.dys, c.blocks, c.scales, c.off)
    pkg.grad_moe_grouped_linear_b_into(want_db, c.dys, c.off)
    xs, bias = c.xs.clone().requires_grad_(True), c.bias.clone().requires_grad_(True)
    ys = pkg.moe_decode_linear_mxfp4(xs, c.blocks, c.scales, c.off, bias)
    assert ys.requires_grad and _same_bits(ys.detach(), c.fwd(True)) and _same_bits(ys.detach(), pkg._moe_decode_linear_mxfp4(c.xs, c.blocks, c.scales, c.off, c.bias))
    assert [(tuple(t.shape), t.dtype) for t in ys.grad_fn.saved_tensors] == [(tuple(c.blocks.shape), torch.uint8), (tuple(c.scales.shape), torch.uint8),
                                                                             ((c.E + 1,), torch.int32)]    # blocks, scales, offsets: no xs, no bias
    ys.backward(c.dys)
    assert _same_bits(xs.grad, want_dxs) and _same_bits(bias.grad, want_db)
    # only what asks for a gradient is computed; without a bias there is none
    x1 = c.xs.clone().requires_grad_(True)
    pkg.moe_decode_linear_mxfp4(x1, c.blocks, c.scales, c.off, c.bias).backward(c.dys)
    assert _same_bits(x1.grad, want_dxs) and c.bias.grad is None
    b1 = c.bias.clone().requires_grad_(True)
    pkg.moe_decode_linear_mxfp4(c.xs, c.blocks, c.scales, c.off, b1).backward(c.dys)
    assert _same_bits(b1.grad, want_db) and c.xs.grad is None
    assert pkg.moe_mx_decode._MoeDecodeLinearMxfp4.backward(None, None) == (None,) * 5
    with torch.no_grad():
        y0 = pkg.moe_decode_linear_mxfp4(xs, c.blocks, c.scales, c.off, bias)
    assert y0.grad_fn is None and not y0.requires_grad and _same_bits(y0, ys.detach())


@pytest.mark.parametrize("dt,K,N,plan", [("bf16", 544, 264, 5), ("f16", 160, 5, 7)])
def test_bitwise_reproducibility(pkg, dt, K, N, plan):
    counts, tail = PLANS[plan]
    c = Case(pkg, plan, counts, tail, K, N, dt)
    assert _same_bits(c.fwd(True), c.fwd(True))


def test_the_forward_is_captured_in_a_graph(pkg):
    """captured on one stream, without parallel branches, and replayed once: the replay equals the eager run bit for bit"""
    counts, tail = PLANS[5]
    c = Case(pkg, 31, counts, tail, 96, 136, "bf16")
    run = lambda: pkg._moe_decode_linear_mxfp4(c.xs, c.blocks, c.scales, c.off, c.bias)
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
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert _same_bits(captured, eager)
