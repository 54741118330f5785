"""GPU tests of the MXFP4 expert weights (include/nnop_hip_moe_mx.h).  The format is judged against tests/mx_ref.py byte for byte and bit
for bit; the two products are judged twice: bit for bit against the sixth library on the dequantised weights (the contract: only the
staging of the weights differs), and against the fp64 formulas of tests/moe_linear_ref.py on mx_ref's dequantised values under the
derived gates of that file, which does not pass through the project's own GEMM or dequantiser.  Every comparison logs error / gate
through util.record_error.

Shapes are the smallest at which the kernels can still go wrong.  A block is 32 values, a reduction step 64, the output tile 128 x 128:
(K, N) = (32, 8) is one block, half a step; (64, 24) one full step; (96, 136) a ragged last step and two column tiles; (544, 264)
17 blocks, nine steps, three column tiles -- for bwd_x five column tiles of K with a ragged one and a reduction over 264; (160, 5) an odd
N: the element-wise output path forward, a reduction of 5 in bwd_x.  The plans are those of tests/test_zzzzzzz_moe_linear_gpu.py; row
strides are dim, dim + 3 and dim + 8; the padding columns hold 7.0 on input and NaN in an output before the call.  Weights are random
codes with scale bytes uniform in 119 ... 131 (|w| <= 96), so sums stay far from the overflow of float16.

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
KNS = ((32, 8), (64, 24), (96, 136), (544, 264), (160, 5))
PADS = (0, 3, 8)
DTS = ("f16", "bf16")
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
        assert {c[4] for c in _mine if c[3] == _pad} == set(range(len(PLANS)))


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
        record_error("moe_mx", dict(name=n, case=case, dt=dt, worst_ratio=r))
    assert all(r <= 1.0 for r in ratios.values()), (case, dt, ratios)


def _out(shape, ld, dt):
    """an output buffer shape[:-1] + (ld,) that holds NaN everywhere, padding columns included -> (the view, the buffer)"""
    buf = torch.full(tuple(shape[:-1]) + (ld,), NAN, dtype=TORCH_DT[dt], device=DEV)
    return buf[..., :shape[-1]], buf


def _padding_kept(buf, dim):
    return bool((_bits(buf[..., dim:]) == _bits(torch.full_like(buf[..., dim:], NAN))).all())


class Case:
    """the inputs of one shape on the device, the packed weights and their dequantised copy, and the two products of either library run
    into pre-filled buffers"""

    def __init__(self, pkg, seed, counts, tail, K, N, dt, pad=0, offsets=None, scales=None):
        self.pkg = pkg
        self.off_np = ref.offsets_of(counts) if offsets is None else np.asarray(offsets, np.int32)
        self.E, self.S, self.K, self.N, self.dt, self.pad = len(counts), int(sum(counts)) + tail, K, N, dt, pad
        self.off = _dev(self.off_np)
        E, S = self.E, self.S
        mk = lambda s, shape: _dev(ref.make(seed + s, shape, dt, shape[-1] + pad), dt)[..., :shape[-1]]
        self.xs, self.dys, self.bias = mk(1, (S, K)), mk(2, (S, N)), mk(4, (E, N))
        self.blocks_np, self.scales_np = mx_ref.random_packed(seed + 3, (E, N, K))
        if scales is not None:
            scales(self.scales_np)
        self.set_weights()
        self._refs = {}

    def set_weights(self):
        self.blocks, self.scales = _dev(self.blocks_np), _dev(self.scales_np)
        self.w = self.pkg.mxfp4_dequantize(self.blocks, self.scales, TORCH_DT[self.dt])          # [E, N, K]: what the sixth library reads

    # ---- the calls: every element in range is written, the padding keeps its NaN ----
    def fwd(self, packed, bias, **over):
        ys, buf = _out((self.S, self.N), self.N + self.pad, self.dt)
        b = over.get("b", self.bias) if bias else None
        xs = over.get("xs", self.xs)
        if packed:
            assert self.pkg.moe_grouped_linear_mxfp4_into(ys, xs, self.blocks, self.scales, self.off, b) is ys
        else:
            self.pkg.moe_grouped_linear_into(ys, xs, self.w, self.off, b, layout="nk")
        assert _padding_kept(buf, self.N)
        return ys

    def bwd_x(self, packed, **over):
        dxs, buf = _out((self.S, self.K), self.K + self.pad, self.dt)
        dys = over.get("dys", self.dys)
        if packed:
            assert self.pkg.grad_moe_grouped_linear_mxfp4_x_into(dxs, dys, self.blocks.view(self.E, self.N, self.K // 2), self.scales, self.off) is dxs
        else:
            self.pkg.grad_moe_grouped_linear_x_into(dxs, dys, self.w, self.off, layout="nk")
        assert _padding_kept(buf, self.K)
        return dxs

    # ---- the fp64 references on mx_ref's weights, each computed once ----
    def refs(self, what):
        if what not in self._refs:
            w = mx_ref.dequant(self.blocks_np, self.scales_np, self.dt)
            xs, dys, b = _np(self.xs), _np(self.dys), _np(self.bias)
            self._refs[what] = {"ys": lambda: ref.linear_ref(xs, w, self.off_np, b), "ys0": lambda: ref.linear_ref(xs, w, self.off_np, None),
                                "dxs": lambda: ref.bwd_x_ref(dys, w, self.off_np)}[what]()
        return self._refs[what]

    def outside(self):
        return torch.tensor(ref.rows_of(self.off_np, self.S) < 0).to(DEV)

    def ys_ratio(self, ys, bias):
        want, A, B = self.refs("ys" if bias else "ys0")
        return ref.worst(ref.fwd_ratios(_np(ys), want, A, B, self.K, self.dt))

    def dxs_ratio(self, dxs):
        want, A = self.refs("dxs")
        return ref.g.ratio(_np(dxs), want, A, self.N, self.dt)


# ---- the format ---------------------------------------------------------------------------------------------------------------------------
def test_exhaustive_table(pkg):
    """every (code, scale byte) pair in the three types against mx_ref, bit for bit: 4096 pairs x 3.  Row e holds the 16 codes twice at the
    scale byte e; the NaNs of row 255 are compared as NaN.  This is the test that decides whether the hardware conversion may be
    used (csrc/moe_mx.hip): it is used for every scale byte."""
    codes = np.tile(np.arange(16, dtype=np.uint8), (256, 1, 2))
    blocks_np, scales_np = mx_ref.pack(codes), np.arange(256, dtype=np.uint8).reshape(256, 1)
    assert blocks_np.shape == (256, 1, 16)
    blocks, scales = _dev(blocks_np), _dev(scales_np)
    bad = {}
    for dt in ("f32", "f16", "bf16"):
        got = pkg.mxfp4_dequantize(blocks, scales, TORCH_DT[dt])
        want = _dev(mx_ref.dequant(blocks_np, scales_np, dt), dt)
        assert got.shape == want.shape == (256, 32) and got.dtype == TORCH_DT[dt]
        assert torch.isnan(got[255]).all() and torch.isnan(want[255]).all() and not torch.isnan(want[:255]).any()
        wrong = (_bits(got[:255]) != _bits(want[:255])).any(dim=1).nonzero().flatten().tolist()
        print(f"exhaustive table [{dt}]: scale bytes with a wrong value: {wrong}")
        record_error("moe_mx", dict(name="table", case="exhaustive", dt=dt, wrong_scale_bytes=wrong))
        if wrong:
            bad[dt] = wrong
    assert not bad, bad


def _quant_inputs(shape, dt, power):
    """normal data times 2^power, rounded to dt, with the special blocks of the header's quantiser: row 1 starts with the tie points
    beside a 6, row 2 with a zero block of mixed signs, row 3 holds one Inf, row 4 one NaN; float16: row 0 is subnormal"""
    rows, K = shape
    rng = np.random.default_rng(rows * K + power)
    x = (3.0 * rng.standard_normal(shape) * 2.0 ** power).astype(np.float32)
    x[1, :16] = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, 0.0]) * 2.0 ** (power + 3)
    x[1, 16:32] = 0.0
    x[2, :32] = np.where(np.arange(32) % 3 == 0, -0.0, 0.0)
    x[3, K - 1], x[4, 0] = np.inf, np.nan
    if dt == "f16" and power == 0:
        x[0] = rng.integers(-1023, 1024, size=K) * 2.0 ** -24
    return torch.tensor(x).to(TORCH_DT[dt])


@pytest.mark.parametrize("dt,power", [("f32", 0), ("f16", 0), ("bf16", 0), ("f32", 60), ("f32", -60), ("bf16", 60), ("bf16", -60)])
@pytest.mark.parametrize("shape", [(37, 96), (5, 32)])
def test_quantiser(pkg, shape, dt, power):
    """mxfp4_quantize against mx_ref.quant, byte for byte; a padded input (ld = K + 8) gives the same bytes and keeps its padding"""
    rows, K = shape
    x = _quant_inputs(shape, dt, power)
    want_b, want_s = mx_ref.quant(x.double().numpy())
    assert (want_s[3, -1], want_s[4, 0], want_s[2, 0]) == (255, 255, 0) and (dt != "f16" or power or want_s[0].max() < 127 - 14)
    blocks, scales = pkg.mxfp4_quantize(x.to(DEV))
    assert blocks.shape == (rows, K // 32, 16) and scales.shape == (rows, K // 32) and blocks.dtype == scales.dtype == torch.uint8
    np.testing.assert_array_equal(scales.cpu().numpy(), want_s)
    np.testing.assert_array_equal(blocks.cpu().numpy(), want_b)
    buf = torch.full((rows, K + 8), 7.0, dtype=x.dtype, device=DEV)
    buf[:, :K] = x.to(DEV)
    before = buf.clone()
    b2, s2 = pkg.mxfp4_quantize(buf[:, :K])
    assert _same_bits(b2, blocks) and _same_bits(s2, scales) and _same_bits(buf, before)
    # what the quantiser wrote comes back from the dequantiser as mx_ref's values (NaN blocks as NaN)
    back = pkg.mxfp4_dequantize(blocks, scales, torch.float32)
    np.testing.assert_array_equal(back.cpu().numpy(), mx_ref.dequant(want_b, want_s, "f32").astype(np.float32))


# ---- the two products ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,dt,pad,plan", GRID, ids=[f"K{c[0]}-N{c[1]}-{c[2]}-pad{c[3]}-plan{c[4]}" for c in GRID])
def test_grid(pkg, K, N, dt, pad, plan):
    """with and without bias, forward and bwd_x: inside the derived gates of the fp64 formulas on mx_ref's weights, and equal to the sixth
    library on the dequantised weights bit for bit; rows outside every expert are +0"""
    counts, tail = PLANS[plan]
    c = Case(pkg, 1000 * K + 10 * N + plan, counts, tail, K, N, dt, pad)
    np.testing.assert_array_equal(_np(c.w), mx_ref.dequant(c.blocks_np, c.scales_np, dt))
    rows, r, same = c.outside(), {}, {}
    for bias in (False, True):
        ys = c.fwd(True, bias)
        r[f"ys-{'b' if bias else '0'}"] = c.ys_ratio(ys, bias)
        same[f"ys-{'b' if bias else '0'}"] = _same_bits(ys, c.fwd(False, bias))
        assert (_bits(ys)[rows] == 0).all()
    dxs = c.bwd_x(True)
    r["dxs"] = c.dxs_ratio(dxs)
    same["dxs"] = _same_bits(dxs, c.bwd_x(False))
    assert (_bits(dxs)[rows] == 0).all()
    print(f"grid [{dt}] bit for bit with the dense path: {same}")
    _log("grid", dt, **r)
    assert all(same.values()), same


# ---- selection and edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_other_experts_and_rows_behind_the_plan_never_enter(pkg, dt):
    """every block of expert 1 carries the scale byte 255 and the rows behind offsets[E] hold NaN: the rows of experts 0 and 2 are finite
    and what they are without either, bit for bit, in both products"""
    K, N = 96, 136
    c = Case(pkg, 5, [17, 65, 30], 20, K, N, dt)
    clean = (c.fwd(True, True), c.bwd_x(True))
    c.scales_np[1] = 255
    c.set_weights()
    xs, dys = c.xs.clone(), c.dys.clone()
    xs[112:], dys[112:] = NAN, NAN
    ys, dxs = c.fwd(True, True, xs=xs), c.bwd_x(True, dys=dys)
    for got, want in ((ys, clean[0]), (dxs, clean[1])):
        for lo, hi in ((0, 17), (82, 112)):
            assert torch.isfinite(got[lo:hi]).all() and _same_bits(got[lo:hi], want[lo:hi])
        assert torch.isnan(got[17:82]).all() and (_bits(got[112:]) == 0).all()                 # the NaNs did arrive where they belong


@pytest.mark.parametrize("dt", DTS)
def test_a_nan_scale_reaches_exactly_what_depends_on_it(pkg, dt):
    """scales[1][n0][b0] = 255: forward, column n0 of expert 1's rows is NaN; bwd_x, columns 32 b0 ... 32 b0 + 31 of those rows; everything
    else keeps its bits"""
    K, N, n0, b0 = 160, 24, 13, 3
    c = Case(pkg, 6, [40, 70, 19], 0, K, N, dt)
    clean = (c.fwd(True, False), c.bwd_x(True))
    c.scales_np[1, n0, b0] = 255
    c.set_weights()
    ys, dxs = c.fwd(True, False), c.bwd_x(True)
    hit_y, hit_x = torch.zeros_like(ys, dtype=torch.bool), torch.zeros_like(dxs, dtype=torch.bool)
    hit_y[40:110, n0], hit_x[40:110, 32 * b0:32 * b0 + 32] = True, True
    for got, want, hit in ((ys, clean[0], hit_y), (dxs, clean[1], hit_x)):
        assert torch.isnan(got[hit]).all() and torch.equal(_bits(got)[~hit], _bits(want)[~hit])


@pytest.mark.parametrize("dt", DTS)
def test_edge_scale_bytes_agree_with_the_dense_path(pkg, dt):
    """scale bytes 0, 1 (subnormal or zero weights), 253, 254 (overflow to Inf) and a few around the range of the hardware conversion
    among the ordinary ones: both products equal dequantise-then-linear bit for bit, NaN patterns included"""
    def edges(s):
        flat = s.reshape(-1)
        flat[::3] = np.resize(np.array([0, 1, 2, 113, 114, 140, 141, 252, 253, 254], np.uint8), flat[::3].size)
    c = Case(pkg, 7, [33, 64, 5], 3, 96, 40, dt, scales=edges)
    assert {0, 254} <= set(c.scales_np.reshape(-1).tolist())
    np.testing.assert_array_equal(_np(c.w), mx_ref.dequant(c.blocks_np, c.scales_np, dt))
    assert torch.isinf(c.w).any() and (dt != "f16" or (c.w[c.w != 0].abs().min() < 2.0 ** -14))
    for bias in (False, True):
        assert _same_bits(c.fwd(True, bias), c.fwd(False, bias)), bias
    assert _same_bits(c.bwd_x(True), c.bwd_x(False))


@pytest.mark.parametrize("offsets", [[-7, 20, 90, 155], [-(2 ** 31), -1, 149, 2 ** 31 - 1], [3, 20, 150, 150], [120, 60, 140, 10]])
def test_out_of_range_offsets_touch_nothing_outside(pkg, offsets):
    """entries below 0, above S, and decreasing: a guard band of NaN rows on either side of both outputs is untouched; with non-decreasing
    entries the result is the dense path's with the same (clamped) ranges"""
    S, E, K, N, G, dt = 150, 3, 96, 136, 130, "bf16"
    c = Case(pkg, 11, [50] * E, 0, K, N, dt, offsets=offsets)
    full = lambda *s: torch.full(s, NAN, dtype=TORCH_DT[dt], device=DEV)
    ys_b, dxs_b = full(G + S + G, N), full(G + S + G, K)
    guard = [_bits(b).clone() for b in (ys_b, dxs_b)]
    ys, dxs = ys_b[G:G + S], dxs_b[G:G + S]
    pkg.moe_grouped_linear_mxfp4_into(ys, c.xs, c.blocks, c.scales, c.off, c.bias)
    pkg.grad_moe_grouped_linear_mxfp4_x_into(dxs, c.dys, c.blocks, c.scales, c.off)
    torch.cuda.synchronize()
    for b, g in zip((ys_b, dxs_b), guard):
        now = _bits(b)
        assert torch.equal(now[:G], g[:G]) and torch.equal(now[G + S:], g[G + S:])
    if offsets == sorted(offsets):
        assert _same_bits(ys, c.fwd(False, True)) and _same_bits(dxs, c.bwd_x(False))
        _log("clamped", dt, ys=c.ys_ratio(ys, True), dxs=c.dxs_ratio(dxs))
        rows = c.outside()
        assert (_bits(ys)[rows] == 0).all() and (_bits(dxs)[rows] == 0).all()


# ---- autograd, reproducibility, capture ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_autograd_gives_the_gradients_of_the_into_calls(pkg, dt):
    counts, tail = PLANS[3]
    c = Case(pkg, 21, counts, tail, 96, 40, dt)
    want_dxs = c.bwd_x(True)
    want_db = torch.empty_like(c.bias)
    pkg.grad_moe_grouped_linear_b_into(want_db, c.dys, c.off)
    xs, bias = c.xs.clone().requires_grad_(True), c.bias.clone().requires_grad_(True)
    ys = pkg.moe_grouped_linear_mxfp4(xs, c.blocks, c.scales, c.off, bias)
    assert ys.requires_grad and _same_bits(ys.detach(), c.fwd(True, True)) and _same_bits(ys.detach(), pkg._moe_grouped_linear_mxfp4(c.xs, c.blocks, c.scales, c.off, c.bias))
    assert [(tuple(t.shape), t.dtype) for t in ys.grad_fn.saved_tensors] == [(tuple(c.blocks.shape), torch.uint8), (tuple(c.scales.shape), torch.uint8),
                                                                             ((c.E + 1,), torch.int32)]    # blocks, scales, offsets: no xs, no bias
    ys.backward(c.dys)
    assert _same_bits(xs.grad, want_dxs) and _same_bits(bias.grad, want_db)
    # only what asks for a gradient is computed; without a bias there is none
    x1 = c.xs.clone().requires_grad_(True)
    pkg.moe_grouped_linear_mxfp4(x1, c.blocks, c.scales, c.off, c.bias).backward(c.dys)
    assert _same_bits(x1.grad, want_dxs) and c.bias.grad is None
    b1 = c.bias.clone().requires_grad_(True)
    pkg.moe_grouped_linear_mxfp4(c.xs, c.blocks, c.scales, c.off, b1).backward(c.dys)
    assert _same_bits(b1.grad, want_db) and c.xs.grad is None
    x2 = c.xs.clone().requires_grad_(True)
    pkg.moe_grouped_linear_mxfp4(x2, c.blocks, c.scales, c.off).backward(c.dys)
    assert _same_bits(x2.grad, want_dxs)
    assert pkg.moe_mx._MoeGroupedLinearMxfp4.backward(None, None) == (None,) * 5
    with torch.no_grad():
        y0 = pkg.moe_grouped_linear_mxfp4(xs, c.blocks, c.scales, c.off, bias)
    assert y0.grad_fn is None and not y0.requires_grad and _same_bits(y0, ys.detach())


@pytest.mark.parametrize("dt,K,N,plan", [("bf16", 544, 264, 3), ("f16", 160, 5, 4)])
def test_bitwise_reproducibility(pkg, dt, K, N, plan):
    counts, tail = PLANS[plan]
    c = Case(pkg, plan, counts, tail, K, N, dt)
    first = (c.fwd(True, True), c.bwd_x(True))
    for a, b in zip((c.fwd(True, True), c.bwd_x(True)), first):
        assert _same_bits(a, b)


def test_forward_and_bwd_x_are_captured_in_a_graph(pkg):
    """the forward and bwd_x on packed weights, captured on one stream and replayed once: the replay equals the eager run bit for bit"""
    counts, tail = PLANS[3]
    c = Case(pkg, 31, counts, tail, 96, 136, "bf16")

    def run():
        ys = pkg._moe_grouped_linear_mxfp4(c.xs, c.blocks, c.scales, c.off, c.bias)
        dxs = torch.empty_like(c.xs)
        pkg.grad_moe_grouped_linear_mxfp4_x_into(dxs, c.dys, c.blocks, c.scales, c.off)
        return dict(ys=ys, dxs=dxs)

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
    for name in ("ys", "dxs"):
        assert _same_bits(captured[name], eager[name]), name
