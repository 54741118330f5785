"""GPU tests of the decode expert forward with the gated activation in its epilogue and the token gather in front
(include/nnop_hip_moe_mx_decode_glu.h).  Results are judged against the fp64 formula of tests/moe_mx_glu_ref.py under the derived gate of
that file, which depends on no summation order and passes through neither the project's GEMM, its dequantiser nor its activation; what the
header promises bit for bit (rows outside the experts, padding, the two layouts, the gather, batch invariance, selection, clamped
offsets, exact data against the two-call form, reproducibility, the gradients) is compared bit for bit.  Every ratio is logged through
util.record_error("moe_mx_decode_glu", ...).

Shapes (K, I) are the smallest at which this kernel can still go wrong.  A block is 32 values, a reduction step 128, the ring holds 2
steps, an MFMA tile is 16 weight rows, a wave owns 64 weight rows and a workgroup 256 = 128 columns of h: (32, 4) is one block; (64, 12)
half a step; (96, 68) a ragged step and three waves; (544, 132) 17 blocks -- five steps, a ragged last one, an odd count for the ring --
two workgroups per expert, and in the halves layout the up rows start at 132, no multiple of 16; (160, 5) an odd I: element-wise stores
and an odd row offset; (2880, 24) the K of gpt-oss: the ring wraps.  The plans are those of tests/test_zzzzzzzzzz_moe_mx_decode_gpu.py:
experts of 0, 1, 16, 17, 31, 33, 63, 64, 65 and 700 rows, rows behind the last expert, an empty first expert.  Row strides are dim,
dim + 3 and dim + 8; the padding columns hold 7.0 on input and NaN in an output before the call.  Weights are mx_ref.random_packed's; x is
scaled by a power of two chosen from the fp64 reference (moe_mx_glu_ref.x_scale) so that the pre-activations have a standard deviation
near 5 -- with unit-scale rows every swiglu_oai element saturates and a test sees nothing; where a case has at least 1024 outputs inside
the experts the reference must show each of gate > limit, up > limit, up < -limit at 2 % of them or more.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

import glu_ref
import moe_linear_ref as lin
import moe_mx_glu_ref as ref
import mx_ref
from util import TORCH_DT, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KIS = ((32, 4), (64, 12), (96, 68), (544, 132), (160, 5), (2880, 24))
PADS = (0, 3, 8)
DTS = ("f16", "bf16")
ACTS = glu_ref.ACTS
NAN = float("nan")
# (counts per expert, rows behind the last expert): the PLANS of tests/test_zzzzzzzzzz_moe_mx_decode_gpu.py
PLANS = (([1], 0), ([0, 2, 0], 0), ([3, 0, 1, 2], 2), ([16], 0), ([17], 0), ([1, 15, 16, 17, 31, 33, 63, 64], 1), ([0, 0, 65], 40),
         ([700, 0, 3], 0))


def _grid():
    """swiglu_oai over every ((K, I), layout, dtype, pad), the plans cycling so that every plan occurs with every layout, dtype and pad;
    the other three activations at (96, 68) and (544, 132) in both layouts and types, pads and plans cycling"""
    cases = []
    for (i, ki), (l, lay), (j, dt), (v, pad) in itertools.product(enumerate(KIS), enumerate(ref.LAYOUTS), enumerate(DTS), enumerate(PADS)):
        cases.append((ki[0], ki[1], "swiglu_oai", lay, dt, pad, (i + 5 * l + 4 * j + 3 * v) % len(PLANS)))
    n = 0
    for act, ki, lay, dt in itertools.product(ACTS[:3], (KIS[2], KIS[3]), ref.LAYOUTS, DTS):
        cases.append((ki[0], ki[1], act, lay, dt, PADS[n % 3], (3 * n + 5) % len(PLANS)))
        n += 1
    return cases


GRID = _grid()
for _lay, _dt, _pad in itertools.product(ref.LAYOUTS, DTS, PADS):
    assert {c[6] for c in GRID if c[3] == _lay and c[2] == "swiglu_oai"} == set(range(len(PLANS)))
    assert {c[6] for c in GRID if c[4] == _dt and c[2] == "swiglu_oai"} == set(range(len(PLANS)))
    assert {c[6] for c in GRID if c[5] == _pad and c[2] == "swiglu_oai"} == set(range(len(PLANS)))


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
        record_error("moe_mx_decode_glu", dict(name=n, case=case, dt=dt, worst_ratio=r))
    assert all(r <= 1.0 for r in ratios.values()), (case, dt, ratios)


class Case:
    """the inputs of one shape on the device, the packed weights, the fp64 reference, and the fused forward run into a NaN-filled padded
    buffer"""

    def __init__(self, pkg, seed, counts, tail, K, I, dt, pad=0, act="swiglu_oai", layout="interleaved", offsets=None):
        self.pkg, self.act, self.layout = pkg, act, layout
        self.off_np = lin.offsets_of(counts) if offsets is None else np.asarray(offsets, np.int32)
        self.E, self.S, self.K, self.I, self.dt, self.pad = len(counts), int(sum(counts)) + tail, K, I, dt, pad
        self.off = _dev(self.off_np)
        self.blocks_np, self.scales_np = mx_ref.random_packed(seed + 3, (self.E, 2 * I, K))
        self.w = mx_ref.dequant(self.blocks_np, self.scales_np, dt)
        x = lin.make(seed + 1, (self.S, K), dt, K + pad)
        self.x_scale = ref.x_scale(x[:, :K], self.w, self.off_np, layout)
        x *= np.float32(self.x_scale)                                      # a power of two: still values of the type
        x[:, K:] = 7.0
        self.x = _dev(x, dt)[:, :K]
        self.bias = _dev(lin.make(seed + 4, (self.E, 2 * I), dt, 2 * I + pad), dt)[:, :2 * I]
        self.set_weights()
        self._refs = {}

    def set_weights(self):
        self.blocks, self.scales = _dev(self.blocks_np), _dev(self.scales_np)

    def kw(self):
        return dict(act=self.act, layout=self.layout)

    def fwd(self, bias, x=None, off=None, **kw):
        """every element in range is written, the padding keeps its NaN"""
        S = self.S if "perm" not in kw else kw["perm"].numel()
        buf = torch.full((S, self.I + self.pad), NAN, dtype=TORCH_DT[self.dt], device=DEV)
        h = buf[:, :self.I]
        got = self.pkg.moe_decode_glu_mxfp4_into(h, self.x if x is None else x, self.blocks, self.scales, self.off if off is None else off,
                                                 self.bias if bias else None, **self.kw(), **kw)
        assert got is h
        assert bool((_bits(buf[:, self.I:]) == _bits(torch.full_like(buf[:, self.I:], NAN))).all())
        return h

    def two_calls(self, bias, x=None):
        """the composition the fused call replaces"""
        gu = self.pkg.moe_decode_linear_mxfp4(self.x if x is None else x, self.blocks, self.scales, self.off, self.bias if bias else None)
        return self.pkg.glu_packed(gu, **self.kw())

    def ref(self, bias):
        if bias not in self._refs:
            self._refs[bias] = ref.glu_decode_ref(_np(self.x), self.w, self.off_np, _np(self.bias) if bias else None, self.act, self.layout)
        return self._refs[bias]

    def ratio(self, h, bias):
        return ref.worst(_np(h), self.ref(bias), self.dt)

    def inside(self):
        return lin.rows_of(self.off_np, self.S) >= 0

    def outside(self):
        return torch.tensor(~self.inside()).to(DEV)


# ---- the grid, and the root-mean-square error against the two-call form -----------------------------------------------------------------
@pytest.mark.parametrize("K,I,act,layout,dt,pad,plan", GRID, ids=[f"K{c[0]}-I{c[1]}-{c[2]}-{c[3]}-{c[4]}-pad{c[5]}-plan{c[6]}" for c in GRID])
def test_grid(pkg, K, I, act, layout, dt, pad, plan):
    """with and without bias: inside the derived gate of the fp64 formula, rows outside every expert all bits zero, padding kept.  Where the
    case has at least 1024 output elements inside the experts: the reference saturates on each side (swiglu_oai), and the
    root-mean-square error of h against fp64 is not above that of glu_packed(moe_decode_linear_mxfp4(...)) on the same inputs, with no
    margin: the fused form drops one rounding and adds none"""
    counts, tail = PLANS[plan]
    c = Case(pkg, 1000 * K + 10 * I + plan, counts, tail, K, I, dt, pad, act, layout)
    rows, inside, r = c.outside(), c.inside(), {}
    big = int(inside.sum()) * I >= 1024
    for bias in (False, True):
        h = c.fwd(bias)
        tag = "b" if bias else "0"
        r[f"h-{tag}"] = c.ratio(h, bias)
        assert (_bits(h)[rows] == 0).all()
        if big:
            want = c.ref(bias)
            if act == "swiglu_oai":
                sat = ref.saturation(want, inside=inside)
                print(f"saturation gate > limit, up > limit, up < -limit: {sat}")
                assert min(sat) >= 0.02, sat
            fused, two = ref.rms(_np(h)[inside], {"h": want["h"][inside]}), ref.rms(_np(c.two_calls(bias))[inside], {"h": want["h"][inside]})
            print(f"rms-{tag} [{dt}] fused {fused:.6e} two calls {two:.6e} ratio {fused / two:.4f}")
            record_error("moe_mx_decode_glu", dict(name=f"rms-{tag}", case="grid", dt=dt, fused=fused, two_calls=two))
            assert fused <= two, (fused, two)
    _log("grid", dt, **r)


# ---- exact data: the two-call form bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ref.LAYOUTS)
@pytest.mark.parametrize("dt", DTS)
def test_exact_data_equals_the_two_call_form_bit_for_bit(pkg, dt, layout):
    """codes of 0, +-0.5, +-1 at the scale byte 127, x in {-1, 0, 1}, K = 64, a bias of 0, +-0.5: every pre-activation is a multiple of 0.5
    of magnitude <= 64.5, which both types hold, so rounding it changes nothing and h is glu_packed of the eighth library's result"""
    K, I = 64, 20
    counts, tail = PLANS[5]
    c = Case(pkg, 77, counts, tail, K, I, dt, 0, "swiglu_oai", layout)
    rng = np.random.default_rng(5)
    code_of = np.array([10, 9, 0, 1, 2], np.uint8)                               # -1, -0.5, 0, 0.5, 1
    c.blocks_np = mx_ref.pack(code_of[rng.integers(0, 5, (c.E, 2 * I, K // 32, 32))])
    c.scales_np = np.full((c.E, 2 * I, K // 32), 127, np.uint8)
    c.set_weights()
    x = _dev(rng.integers(-1, 2, (c.S, K)).astype(np.float32), dt)
    c.bias = _dev(rng.integers(-1, 2, (c.E, 2 * I)).astype(np.float32) * 0.5, dt)
    for bias in (False, True):
        gu = pkg.moe_decode_linear_mxfp4(x, c.blocks, c.scales, c.off, c.bias if bias else None)
        assert float(gu.abs().max()) > 8 and bool((gu.float() * 2 == (gu.float() * 2).round()).all())
        for act in ACTS:
            c.act = act
            assert _same_bits(c.fwd(bias, x=x), pkg.glu_packed(gu, act=act, layout=layout)), (act, bias)


# ---- the two layouts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,K,I,plan", [("bf16", 544, 132, 5), ("f16", 160, 5, 2), ("bf16", 96, 68, 6)])
def test_the_two_layouts_give_the_same_bits(pkg, dt, K, I, plan):
    """the halves call on the de-interleaved weights and bias equals the interleaved call bit for bit, on random data"""
    counts, tail = PLANS[plan]
    a = Case(pkg, 91 + plan, counts, tail, K, I, dt, 3, "swiglu_oai", "interleaved")
    b = Case(pkg, 91 + plan, counts, tail, K, I, dt, 3, "swiglu_oai", "halves")
    b.blocks_np, b.scales_np = ref.to_halves(a.blocks_np, 1), ref.to_halves(a.scales_np, 1)
    b.set_weights()
    b.x, b.bias = a.x, _dev(ref.to_halves(_np(a.bias), 1), dt)
    for act in ("swiglu_oai", "gelu_erf"):
        a.act = b.act = act
        for bias in (False, True):
            ha = a.fwd(bias)
            assert torch.isfinite(ha).all() and _same_bits(ha, b.fwd(bias)), (act, bias)


# ---- the gather ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ref.LAYOUTS)
@pytest.mark.parametrize("dt", DTS)
def test_the_gather_equals_moe_permute_in_front(pkg, dt, layout):
    """perm from moe_dispatch_plan over T = 45 tokens, k = 4, E = 6: a token that names one expert twice, assignments the plan skips (-1 and
    E as the expert), one token that no valid entry names and whose row is NaN, and two perm entries overwritten with -1 and T k.  The
    fused call with perm equals moe_permute followed by the call without, bit for bit, and lies inside the gate"""
    T, k, E, K, I = 45, 4, 6, 96, 68
    rng = np.random.default_rng(17)
    idx = np.stack([rng.permutation(E)[:k] for _ in range(T)]).astype(np.int32)
    idx[3] = [2, 2, 5, 0]                                                        # one expert twice
    idx[7, 1], idx[9, 0] = -1, E                                                 # skipped assignments
    idx[11] = -1                                                                 # a token nobody names
    _, off, perm, _ = pkg.moe_dispatch_plan(_dev(idx), E)
    perm = perm.clone()
    valid = torch.nonzero((perm >= 0) & (perm // k != 11)).flatten()
    perm[valid[5]], perm[valid[40]] = -1, T * k
    perm_np = perm.cpu().numpy()
    assert (perm_np == -1).sum() >= 2 and (perm_np == T * k).sum() == 1 and not ((perm_np >= 0) & (perm_np < T * k) & (perm_np // k == 11)).any()
    c = Case(pkg, 23, [T * k // E] * E, 0, K, I, dt, 3, "swiglu_oai", layout, offsets=off.cpu().numpy())
    x = c.x[:T].clone()
    x[11] = NAN
    xs = torch.empty((T * k, K), dtype=x.dtype, device=DEV)
    pkg.moe_permute_into(xs, x, perm)
    assert torch.isfinite(xs).all()
    for bias in (False, True):
        got = c.fwd(bias, x=x, perm=perm, k=k)
        assert torch.isfinite(got).all() and _same_bits(got, c.fwd(bias, x=xs))
        assert _same_bits(got, pkg._moe_decode_glu_mxfp4(x, c.blocks, c.scales, c.off, c.bias if bias else None, layout=layout, perm=perm, k=k))
        want = ref.glu_decode_ref(ref.gather(_np(x), perm_np, k), c.w, c.off_np, _np(c.bias) if bias else None, c.act, layout)
        _log("gather", dt, **{f"h-{'b' if bias else '0'}": ref.worst(_np(got), want, dt)})
    # a row whose perm entry is invalid is the activation of the bias alone
    s = int(valid[5])
    e = int(lin.rows_of(c.off_np, T * k)[s])
    alone = pkg.glu_packed(c.bias[e:e + 1].contiguous(), act="swiglu_oai", layout=layout)
    assert _same_bits(c.fwd(True, x=x, perm=perm, k=k)[s:s + 1], alone)


# ---- batch invariance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ref.LAYOUTS)
@pytest.mark.parametrize("dt", DTS)
def test_a_rows_bits_do_not_depend_on_the_plan_or_the_gather(pkg, dt, layout):
    """the same x rows reach the same experts in two plans over the same weights: at other positions of their expert's range, in another
    row group and another pass (so beside another number of accumulator groups), with other neighbours, another S and other rows in
    front of and behind the experts -- and once more through perm, from a shuffled token array.  Their h bits are equal"""
    K, I = 544, 36
    a = Case(pkg, 41, [5, 20, 3], 0, K, I, dt, 0, "swiglu_oai", layout)
    b = Case(pkg, 43, [40, 37, 0], 2, K, I, dt, 0, "swiglu_oai", layout)
    b.blocks_np, b.scales_np, b.bias = a.blocks_np, a.scales_np, a.bias
    b.set_weights()
    x = (b.x * (a.x_scale / b.x_scale)).clone()
    moves = ((0, 5, 3), (5, 10, 72), (10, 25, 49))
    for lo, hi, to in moves:
        x[to:to + hi - lo] = a.x[lo:hi]
    shuffle = torch.randperm(b.S, generator=torch.Generator().manual_seed(3)).to(DEV)
    tokens = torch.empty_like(x)
    tokens[shuffle] = x                                                          # token shuffle[s] is slot row s
    perm = shuffle.to(torch.int32)
    for bias in (False, True):
        ha, hb, hp = a.fwd(bias), b.fwd(bias, x=x), b.fwd(bias, x=tokens, perm=perm, k=1)
        assert torch.isfinite(ha).all() and _same_bits(hb, hp)
        for lo, hi, to in moves:
            assert _same_bits(ha[lo:hi], hb[to:to + hi - lo]), (bias, lo)
        assert not _same_bits(hb[:5], ha[:5])                        # other rows did give other results
    _log("invariance", dt, h=a.ratio(a.fwd(True), True))


# ---- selection --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ref.LAYOUTS)
@pytest.mark.parametrize("dt", DTS)
def test_experts_without_rows_and_rows_outside_never_enter(pkg, dt, layout):
    """every block of expert 1, which has no rows, carries the scale byte 255 or codes and a scale that give Inf, and the x rows behind
    offsets[E] hold NaN: the rows of experts 0 and 2 are finite and what they are without either, bit for bit; the rows behind +0"""
    c = Case(pkg, 5, [17, 0, 30], 20, 96, 68, dt, 0, "swiglu_oai", layout)
    clean = c.fwd(True)
    c.scales_np[1, ::2], c.scales_np[1, 1::2], c.blocks_np[1, 1::2] = 255, 254, 0x77
    c.set_weights()
    x = c.x.clone()
    x[47:] = NAN
    h = c.fwd(True, x=x)
    assert torch.isfinite(h[:47]).all() and _same_bits(h[:47], clean[:47]) and (_bits(h[47:]) == 0).all()
    # the same with an expert that has rows: the others keep their bits, and its own rows are what nnop_glu makes of NaN pre-activations
    # (swiglu_oai's min and clamp take a NaN to the bound), as in the two-call form
    d = Case(pkg, 5, [17, 3, 27], 20, 96, 68, dt, 0, "swiglu_oai", layout)
    clean = d.fwd(True)
    d.scales_np[1] = 255
    d.set_weights()
    x = d.x.clone()
    x[47:] = NAN
    h = d.fwd(True, x=x)
    assert _same_bits(h[:17], clean[:17]) and _same_bits(h[20:47], clean[20:47]) and (_bits(h[47:]) == 0).all()
    two = d.two_calls(True, x=x)
    assert not _same_bits(h[17:20], clean[17:20]) and _same_bits(h[17:20], two[17:20])


# ---- offsets ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [[-7, 20, 90, 155], [-(2 ** 31), -1, 149, 2 ** 31 - 1], [3, 20, 150, 150], [120, 60, 140, 10]])
def test_out_of_range_offsets_are_clamped_and_touch_nothing_outside(pkg, offsets):
    """entries below 0, above S, and decreasing: the result equals the call with the clamped offsets bit for bit, rows outside the ranges
    are +0, and a guard band of NaN rows on either side of h is untouched"""
    S, E, K, I, G, dt = 150, 3, 96, 68, 130, "bf16"
    for layout in ref.LAYOUTS:
        c = Case(pkg, 11, [50] * E, 0, K, I, dt, 0, "swiglu_oai", layout, offsets=offsets)
        band = torch.full((G + S + G, I), NAN, dtype=TORCH_DT[dt], device=DEV)
        guard = _bits(band).clone()
        h = band[G:G + S]
        pkg.moe_decode_glu_mxfp4_into(h, c.x, c.blocks, c.scales, c.off, c.bias, layout=layout)
        torch.cuda.synchronize()
        now = _bits(band)
        assert torch.equal(now[:G], guard[:G]) and torch.equal(now[G + S:], guard[G + S:])
        clamped = _dev(lin.clamp_offsets(offsets, S).astype(np.int32))
        assert _same_bits(h, c.fwd(True, off=clamped))
        assert (_bits(h)[c.outside()] == 0).all()
        if offsets == sorted(offsets):
            _log("clamped", dt, h=c.ratio(h, True))


# ---- reproducibility, capture, autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,K,I,plan,layout", [("bf16", 544, 132, 5, "interleaved"), ("f16", 160, 5, 7, "halves")])
def test_bitwise_reproducibility(pkg, dt, K, I, plan, layout):
    counts, tail = PLANS[plan]
    c = Case(pkg, plan, counts, tail, K, I, dt, 0, "swiglu_oai", layout)
    assert _same_bits(c.fwd(True), c.fwd(True))


def test_the_forward_is_captured_in_a_graph(pkg):
    """captured on one stream, without parallel branches, and replayed once: the replay equals the eager run bit for bit"""
    counts, tail = PLANS[5]
    c = Case(pkg, 31, counts, tail, 96, 68, "bf16")
    run = lambda: pkg._moe_decode_glu_mxfp4(c.x, c.blocks, c.scales, c.off, c.bias)
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


@pytest.mark.parametrize("act,layout", [("swiglu_oai", "interleaved"), ("silu", "halves"), ("gelu_tanh", "interleaved")])
@pytest.mark.parametrize("dt", DTS)
def test_autograd_gives_the_gradients_of_the_two_call_form(pkg, dt, act, layout):
    """x.grad and bias.grad equal those of glu_packed(moe_decode_linear_mxfp4(x, ..., bias)) bit for bit; saved are blocks, scales, offsets,
    x and the bias, and nothing of size [S, 2 I]"""
    counts, tail = PLANS[5]
    c = Case(pkg, 21, counts, tail, 96, 20, dt, 0, act, layout)
    dh = _dev(lin.make(9, (c.S, c.I), dt), dt)
    x0, b0 = c.x.clone().requires_grad_(True), c.bias.clone().requires_grad_(True)
    pkg.glu_packed(pkg.moe_decode_linear_mxfp4(x0, c.blocks, c.scales, c.off, b0), act=act, layout=layout).backward(dh)
    x, bias = c.x.clone().requires_grad_(True), c.bias.clone().requires_grad_(True)
    h = pkg.moe_decode_glu_mxfp4(x, c.blocks, c.scales, c.off, bias, act=act, layout=layout)
    assert h.requires_grad and _same_bits(h.detach(), c.fwd(True))
    saved = [(tuple(t.shape), t.dtype) for t in h.grad_fn.saved_tensors]
    assert saved == [(tuple(c.blocks.shape), torch.uint8), (tuple(c.scales.shape), torch.uint8), ((c.E + 1,), torch.int32),
                     (tuple(c.x.shape), TORCH_DT[dt]), (tuple(c.bias.shape), TORCH_DT[dt])]
    h.backward(dh)
    assert torch.isfinite(x.grad).all() and bool(x.grad.any()) and _same_bits(x.grad, x0.grad) and _same_bits(bias.grad, b0.grad)
    # only what asks for a gradient is computed; without a bias none is saved
    x1 = c.x.clone().requires_grad_(True)
    h1 = pkg.moe_decode_glu_mxfp4(x1, c.blocks, c.scales, c.off, None, act=act, layout=layout)
    assert len(h1.grad_fn.saved_tensors) == 4
    h1.backward(dh)
    x2 = c.x.clone().requires_grad_(True)
    pkg.glu_packed(pkg.moe_decode_linear_mxfp4(x2, c.blocks, c.scales, c.off), act=act, layout=layout).backward(dh)
    assert _same_bits(x1.grad, x2.grad)
    b1 = c.bias.clone().requires_grad_(True)
    pkg.moe_decode_glu_mxfp4(c.x, c.blocks, c.scales, c.off, b1, act=act, layout=layout).backward(dh)
    assert _same_bits(b1.grad, b0.grad) and c.x.grad is None
    assert pkg.moe_mx_decode_glu._MoeDecodeGluMxfp4.backward(None, None) == (None,) * 9
    with torch.no_grad():
        h0 = pkg.moe_decode_glu_mxfp4(x, c.blocks, c.scales, c.off, bias, act=act, layout=layout)
    assert h0.grad_fn is None and not h0.requires_grad and _same_bits(h0, h.detach())
    perm = torch.arange(c.S, dtype=torch.int32, device=DEV)
    with pytest.raises(pkg.NNopError, match="moe_permute, moe_decode_linear_mxfp4 and glu_packed"):
        pkg.moe_decode_glu_mxfp4(x, c.blocks, c.scales, c.off, bias, act=act, layout=layout, perm=perm, k=1)
