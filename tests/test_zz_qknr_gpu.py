"""GPU tests of the fused QK-norm + RoPE (include/nnop_hip_ext.h) against tests/qknr_ref.py: the header's formulas in fp64 on the rounded
inputs.  Gates are the project's own and are not widened: TOL of tests/test_rope_gpu.py for q_out, k_out, dq, dk with atol scaled by
max(1, max|ref|); the RMSNorm dw gate of tests/test_norms_gpu.py (rtol 1e-4, atol 1e-5 max|ref| + 1e-6 rows) for dwq, dwk.  An fp32
evaluation rounded once reaches at most 0.24 of the output gates and 0.014 of the dw gate on the CPU; what the kernels reach is recorded
in profiles/qknr/parity.json (every comparison logs its ratio through util.record_error).

Shapes are the smallest that reach every path: each D of the 16-byte path (16 ... 512: 1 ... 32 lanes per row) and three of the
element-wise path, L in {1, 37, 257}, three head pairs, one and two batches, position ids that start at 1000 and differ per batch.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

import qknr_ref as ref
from util import TORCH_DT, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
VEC_D, ELEM_D = (16, 32, 64, 128, 256, 512), (6, 80, 96)
LS, HEADS, BS = (1, 37, 257), ((4, 1), (3, 3), (5, 1)), (1, 2)


def _grid():
    """One case per (D, dtype, dtype of w, dtype of cos / sin); L, the head pair, B and offset cycle so that every value of each occurs
    with every dtype (checked below)."""
    cases = []
    for (i, D), (j, dt) in itertools.product(enumerate(VEC_D + ELEM_D), enumerate(("f32", "f16", "bf16"))):
        for v, (w_in_t, cs_in_t) in enumerate(((False, False),) if dt == "f32" else itertools.product((False, True), repeat=2)):
            n = i + j + v
            cases.append((D, dt, w_in_t, cs_in_t, LS[n % 3], HEADS[(i + 2 * j + v // 2) % 3], BS[(i + v) % 2], float((i + j + v // 2) % 2)))
    return cases


GRID = _grid()
for _dt in ("f32", "f16", "bf16"):
    _mine = [c for c in GRID if c[1] == _dt]
    assert {c[0] for c in _mine} == set(VEC_D + ELEM_D) and {c[4] for c in _mine} == set(LS) and {c[5] for c in _mine} == set(HEADS)
    assert {c[6] for c in _mine} == set(BS) and {c[7] for c in _mine} == {0.0, 1.0}
    assert _dt == "f32" or {(c[2], c[3]) for c in _mine} == set(itertools.product((False, True), repeat=2))


def _np(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _dev(x, dt, w_in_t=False, cs_in_t=False):
    """the fp32 numpy inputs of ref.make_inputs on the device: q, k, dq2, dk2 in dt, the weights and the tables in fp32 or dt"""
    tdt = TORCH_DT[dt]
    kind = {"wq": w_in_t, "wk": w_in_t, "cos": cs_in_t, "sin": cs_in_t}
    return {n: torch.tensor(v).to(tdt if kind.get(n, True) else torch.float32).to(DEV) for n, v in x.items()}


def _args(t):
    return t["q"], t["k"], t["wq"], t["wk"], t["cos"], t["sin"]


def _reference(t, offset):
    a = [_np(v) for v in _args(t)]
    return ref.qknr_ref(*a, EPS, offset) + ref.qknr_grad_ref(_np(t["dq2"]), _np(t["dk2"]), *a, EPS, offset)


def _judge(name, got, want, dt, rows_q, rows_k):
    """got, want: (q2, k2, dq, dk, dwq, dwk); every ratio is logged, then all are asserted"""
    ratios = {n: ref.out_ratio(_np(g), w, dt) for n, g, w in zip(("q_out", "k_out", "dq", "dk"), got, want)}
    ratios["dwq"] = ref.dw_ratio(_np(got[4]), want[4], rows_q)
    ratios["dwk"] = ref.dw_ratio(_np(got[5]), want[5], rows_k)
    for n, r in ratios.items():
        print(f"{name} [{dt}] {n}: error / gate = {r:.4f}")
        record_error("qknr", dict(name=n, case=name, dt=dt, worst_ratio=r))
    assert all(r <= 1.0 for r in ratios.values()), (name, dt, ratios)
    return ratios


def _both(pkg, t, offset):
    out = pkg._qk_norm_rope(*_args(t), eps=EPS, offset=offset)
    return out + pkg.grad_qk_norm_rope((t["dq2"], t["dk2"]), *_args(t), eps=EPS, offset=offset)


def _case(pkg, name, seed, B, QH, KH, L, D, dt, w_in_t=False, cs_in_t=False, offset=0.0, scale=1.0):
    t = _dev(ref.make_inputs(seed, B, QH, KH, L, D, scale), dt, w_in_t, cs_in_t)
    got = _both(pkg, t, offset)
    assert got[0].dtype == t["q"].dtype and got[4].dtype == torch.float32 and got[0].shape == t["q"].shape and got[5].shape == (D,)
    _judge(name, got, _reference(t, offset), dt, B * QH * L, B * KH * L)
    return t, got


@pytest.mark.parametrize("D,dt,w_in_t,cs_in_t,L,heads,B,offset", GRID,
                         ids=[f"D{c[0]}-{c[1]}-w{'T' if c[2] else '32'}-cs{'T' if c[3] else '32'}-L{c[4]}-H{c[5][0]}x{c[5][1]}-B{c[6]}-o{c[7]:g}" for c in GRID])
def test_grid(pkg, D, dt, w_in_t, cs_in_t, L, heads, B, offset):
    _case(pkg, "grid", D * 1000 + L, B, heads[0], heads[1], L, D, dt, w_in_t, cs_in_t, offset)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("scale", [1e-3, 30.0])
def test_input_scales(pkg, dt, scale):
    _case(pkg, f"scale{scale:g}", 5, 2, 4, 1, 37, 128, dt, offset=1.0, scale=scale)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_item_tail_does_not_fill_the_last_wave(pkg, dt):
    """L = 37, D = 64: 148 head rows of 4 lanes = 592 items, 16 lanes into the last wave; the other 48 work on a clamped row and store nothing"""
    B, QH, KH, L, D = 1, 3, 1, 37, 64
    assert (B * (QH + KH) * L * (D // 16)) % 64 == 16
    # the outputs sit in front of a guard band that must stay untouched
    t = _dev(ref.make_inputs(3, B, QH, KH, L, D), dt)
    want = _reference(t, 0.0)
    guard = 4096
    bufs = [torch.full((n + guard,), 7.0, dtype=t["q"].dtype, device=DEV) for n in (t["q"].numel(), t["k"].numel()) * 2]
    outs = [b[:b.numel() - guard].view(s.shape) for b, s in zip(bufs, (t["q"], t["k"]) * 2)]
    dw = [torch.empty(D, dtype=torch.float32, device=DEV) for _ in range(2)]
    pkg.qk_norm_rope_into(outs[0], outs[1], *_args(t), eps=EPS)
    pkg.grad_qk_norm_rope_into(outs[2], outs[3], dw[0], dw[1], (t["dq2"], t["dk2"]), *_args(t), eps=EPS)
    _judge("tail", outs + dw, want, dt, B * QH * L, B * KH * L)
    for b in bufs:
        assert (b[b.numel() - guard:] == 7.0).all()


def _misaligned_like(t):
    flat = torch.empty(t.numel() + 2, dtype=t.dtype, device=t.device)
    view = flat[1:1 + t.numel()].view(t.shape)                      # one element (2 or 4 bytes) past a 16-byte boundary
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    view.copy_(t)
    return view


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("which", ["q", "wk", "cos", "out", "dq2"])
def test_base_offset_by_one_element_takes_the_element_path(pkg, dt, which):
    B, QH, KH, L, D = 2, 3, 2, 37, 64
    t = _dev(ref.make_inputs(77, B, QH, KH, L, D), dt)
    want = _reference(t, 1.0)
    outs = [torch.empty_like(t[n]) for n in ("q", "k", "q", "k")]
    dw = [torch.empty(D, dtype=torch.float32, device=DEV) for _ in range(2)]
    if which == "out":
        outs[0], outs[3] = _misaligned_like(outs[0]), _misaligned_like(outs[3])
    else:
        t[which] = _misaligned_like(t[which])
    pkg.qk_norm_rope_into(outs[0], outs[1], *_args(t), eps=EPS, offset=1.0)
    pkg.grad_qk_norm_rope_into(outs[2], outs[3], dw[0], dw[1], (t["dq2"], t["dk2"]), *_args(t), eps=EPS, offset=1.0)
    _judge(f"offset-{which}", outs + dw, want, dt, B * QH * L, B * KH * L)


@pytest.mark.parametrize("D", [64, 80, 512])
def test_in_place_is_bitwise_the_out_of_place_result(pkg, D):
    t = _dev(ref.make_inputs(9, 2, 3, 1, 37, D), "bf16")
    keep = {n: t[n].clone() for n in ("q", "k", "dq2", "dk2")}
    got = _both(pkg, t, 1.0)
    assert all(torch.equal(t[n], keep[n]) for n in keep)                # out of place: the inputs are untouched
    dq2, dk2 = t["dq2"].clone(), t["dk2"].clone()
    dw = [torch.empty(D, dtype=torch.float32, device=DEV) for _ in range(2)]
    pkg.grad_qk_norm_rope_into(dq2, dk2, dw[0], dw[1], (dq2, dk2), *_args(t), eps=EPS, offset=1.0)      # dq on dq_out, dk on dk_out
    for a, b in zip((dq2, dk2, dw[0], dw[1]), got[2:]):
        assert torch.equal(a, b)
    pkg.qk_norm_rope_into(t["q"], t["k"], *_args(t), eps=EPS, offset=1.0)                                 # q_out on q, k_out on k
    assert torch.equal(t["q"], got[0]) and torch.equal(t["k"], got[1])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_multi_partial_fold_is_within_the_gate_and_deterministic(pkg, dt):
    """rows far above the partial count: 8248 head rows of q on 33 workgroups x 64 groups, four rows per group and a ragged last round"""
    B, QH, KH, L, D = 2, 4, 1, 1031, 64
    t, got = _case(pkg, "fold", 11, B, QH, KH, L, D, dt, offset=1.0)
    again = _both(pkg, t, 1.0)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def _partials(rows_q, rows_k, lanes_per_row):
    """csrc/qk_norm_rope.hip qknr_parts: a workgroup of 256 / lanes_per_row groups per partial row, four rows of the longer tensor per group"""
    per_partial = 4 * (256 // lanes_per_row)
    return min(1024, max(1, -(-max(rows_q, rows_k) // per_partial)))


@pytest.mark.parametrize("B,QH,KH,L,D,dt,lanes_per_row,parts", [(1, 3, 1, 700, 6, "f32", 64, 132), (2, 4, 1, 4129, 64, "bf16", 4, 130)],
                         ids=["element-path-132-partials", "16-byte-path-130-partials"])
def test_fold_of_more_than_128_partials_is_within_the_gate_and_deterministic(pkg, B, QH, KH, L, D, dt, lanes_per_row, parts):
    """The fold kernel (csrc/row_common.hpp fold_partial_rows_kernel) sums slices of 32 partial rows with four accumulators while more
    than 96 rows are ahead, then one by one: more than 128 partials, no multiple of 128, reach both loops.  k has fewer head rows than q
    and as many partial rows, the last ones all zero.  The second base of the fold (k's partials) is computed on the host."""
    rows_q, rows_k = B * QH * L, B * KH * L
    assert _partials(rows_q, rows_k, lanes_per_row) == parts and parts > 128 and parts % 128 != 0 and rows_k < rows_q
    t, got = _case(pkg, f"fold{parts}", 31, B, QH, KH, L, D, dt, offset=1.0)
    if lanes_per_row == 64:          # the library sizes the workspace by the same rule for the narrowest workgroup: the element path's
        import ctypes as C
        d = pkg.qknorm._desc(t["q"], t["k"], t["wq"], t["cos"], EPS, 1.0)
        assert pkg._lib_ext.load().nnop_qk_norm_rope_bwd_workspace_bytes(C.byref(d)) == parts * 2 * D * 4
    again = _both(pkg, t, 1.0)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("D", [128, 96])
def test_nan_prefilled_workspace_and_outputs_change_nothing(pkg, D):
    B, QH, KH, L = 2, 5, 1, 257
    t = _dev(ref.make_inputs(13, B, QH, KH, L, D), "bf16")
    got = _both(pkg, t, 0.0)
    nan = lambda like, dtype=None: torch.full_like(like, float("nan"), dtype=dtype)
    outs = [nan(t["q"]), nan(t["k"]), nan(t["q"]), nan(t["k"]), nan(t["wq"], torch.float32), nan(t["wk"], torch.float32)]
    d = pkg.qknorm._desc(t["q"], t["k"], t["wq"], t["cos"], EPS, 0.0)
    import ctypes as C
    nbytes = pkg._lib_ext.load().nnop_qk_norm_rope_bwd_workspace_bytes(C.byref(d))
    ws = torch.full((nbytes // 4 + 64,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)
    pkg.qk_norm_rope_into(outs[0], outs[1], *_args(t), eps=EPS)
    pkg.grad_qk_norm_rope_into(*outs[2:], (t["dq2"], t["dk2"]), *_args(t), eps=EPS, workspace=ws)
    for a, b in zip(outs, got):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("D", [64, 6])
def test_single_row(pkg, dt, D):
    _case(pkg, "single", 17, 1, 1, 1, 1, D, dt, offset=1.0)


def test_edge_rows(pkg):
    """an all-zero row gives zeros and finite gradients; an fp16 row of +-3e4 gives a finite y: the squares are taken in fp32"""
    B, QH, KH, L, D = 1, 2, 1, 5, 64
    x = ref.make_inputs(19, B, QH, KH, L, D)
    x["q"][0, 1, 2] = 0.0
    x["k"][0, 0, 3] = 3e4 * np.where(np.arange(D) % 2, -1.0, 1.0)
    t = _dev(x, "f16")
    got = _both(pkg, t, 0.0)
    assert (got[0][0, 1, 2] == 0).all() and all(torch.isfinite(g).all() for g in got)
    assert (got[1][0, 0, 3].abs() > 0).any()
    _judge("edge", got, _reference(t, 0.0), "f16", B * QH * L, B * KH * L)


def test_two_call_parity_f32(pkg):
    """fp32: the fused result against llama_rope(rms_norm(q), rms_norm(k)) of the main library, within 4 x the rope TOL"""
    B, QH, KH, L, D = 2, 4, 1, 37, 128
    t = _dev(ref.make_inputs(23, B, QH, KH, L, D), "f32")
    q2, k2 = pkg._qk_norm_rope(*_args(t), eps=EPS, offset=1.0)
    nq = pkg.rms_norm(t["q"].view(-1, D), t["wq"], eps=EPS, offset=1.0).view_as(t["q"])
    nk = pkg.rms_norm(t["k"].view(-1, D), t["wk"], eps=EPS, offset=1.0).view_as(t["k"])
    sq, sk = pkg.llama_rope(nq, nk, cos=t["cos"], sin=t["sin"])
    tol = {k: 4 * v for k, v in ref.TOL["f32"].items()}
    np.testing.assert_allclose(_np(q2), _np(sq), **tol)
    np.testing.assert_allclose(_np(k2), _np(sk), **tol)


@pytest.mark.parametrize("dt,w_in_t", [("f32", False), ("bf16", True)])
def test_autograd_gives_the_gradients_of_grad_qk_norm_rope(pkg, dt, w_in_t):
    B, QH, KH, L, D = 2, 3, 1, 37, 64
    t = _dev(ref.make_inputs(29, B, QH, KH, L, D), dt, w_in_t)
    leaves = [t[n].clone().requires_grad_(True) for n in ("q", "k", "wq", "wk")]
    q2, k2 = pkg.qk_norm_rope(*leaves, cos=t["cos"], sin=t["sin"], eps=EPS, offset=1.0)
    want = _both(pkg, t, 1.0)
    assert torch.equal(q2, want[0]) and torch.equal(k2, want[1]) and q2.requires_grad
    torch.autograd.backward((q2, k2), (t["dq2"], t["dk2"]))
    for leaf, g in zip(leaves, want[2:]):
        assert leaf.grad.dtype == leaf.dtype and torch.equal(leaf.grad, g.to(leaf.dtype))
    assert t["cos"].grad is None and t["sin"].grad is None
    with torch.no_grad():
        q3, _ = pkg.qk_norm_rope(*leaves, cos=t["cos"], sin=t["sin"], eps=EPS, offset=1.0)
    assert not q3.requires_grad and torch.equal(q3, want[0])
