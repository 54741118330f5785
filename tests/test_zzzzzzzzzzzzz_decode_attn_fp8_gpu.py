"""GPU tests of decode attention over an E4M3 KV cache (include/nnop_hip_decode_attn_fp8.h).  The reference is the tenth library's test's
plain fp64 softmax over the keys a query sees, on the DEQUANTISED cache (code value x scale) and the rounded q, so it holds no
quantisation error and util.py's gates apply as they stand.  Shapes as in that test: capacity 300, lengths at a tile edge, at one round
of the four waves and one beside each, 0, 1 and the capacity, 1 / 3 / 7 splits.  The kernel's ring holds D = 4 tiles per wave
(kDfRing), and a wave consumes a slot that was refilled twice only from 8 D + 1 = 33 tiles per chunk, so the LONG cases have a capacity
of 1100 = 35 tiles at one split.  In every parity case every cache row that no query of its sequence sees holds the NaN code 0x7F.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

from test_zzzzzzzzzzzz_decode_attn_gpu import _f64, _ratio, ref_decode
from util import TORCH_DT, assert_close, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP, LONG_CAP, KH, B = 300, 1100, 2, 3
LENS = (0, 1, 31, 32, 33, 127, 128, 129, CAP)
ROWS = ((1, 1), (5, 1), (16, 1), (8, 2))                 # (G, QL)
WINDOWS = (None, 0, 40, 128)
SPLITS = (1, 3, 7)
SINKS = (None, (-np.inf, 0.7, 30.0))
LAYOUTS = ("bhle", "blhe")
SCALES = (None, ((0.75, 0.013), (1.5, 0.02)))            # (k_scale, v_scale) per KV head: no powers of two
NINF = -np.inf
VALUE = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()      # code -> value; 0x7F and 0xFF are NaN
FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)               # the 254 finite codes

# every (E, type, (G, QL)) three times, the other axes cycling: 48 cases; then the 5 LONG ones
GRID = [(E, dt, G, QL, CAP, (LENS[n % 9], LENS[(2 * n + 3) % 9], LENS[(4 * n + 7) % 9]), SPLITS[(n + n // 9) % 3], WINDOWS[(n // 3) % 4],
         SINKS[(n // 2) % 2], LAYOUTS[(n // 5) % 2], SCALES[(n // 7) % 2])
        for n, (E, dt, (G, QL), _) in enumerate(itertools.product((64, 128), ("f16", "bf16"), ROWS, range(3)))]
assert all({c[i] for c in GRID} == set(vals) for i, vals in ((6, SPLITS), (7, WINDOWS), (8, SINKS), (9, LAYOUTS), (10, SCALES)))
assert {n for c in GRID for n in c[5]} == set(LENS)
GRID += [(E, ("bf16", "f16")[n % 2], 8, 1 + n // 2 % 2, LONG_CAP, (LONG_CAP, 577, 289), splits, window, SINKS[n % 2], LAYOUTS[n // 2 % 2], SCALES[1])
         for n, (E, window, splits) in enumerate([(64, None, 1), (64, 900, 1), (128, None, 1), (128, 900, 1), (128, None, 2)])]

_INPUTS = {}


def _inputs(E, dt, G, QL, layout, cap, scales):
    """q, the two caches (standard normal over the scale, cast to E4M3 on the CPU: scale 1 reaches the subnormal codes) and the scales;
    made once per key and left unchanged (tests clone what they overwrite)"""
    key = (E, dt, G, QL, layout, cap, scales)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * E + 10 * G + QL)
        q = torch.tensor(rng.standard_normal((B, KH * G, QL, E)).astype(np.float32)).to(TORCH_DT[dt]).to(DEV)
        sc = [None if scales is None else torch.tensor(s, dtype=torch.float32) for s in (scales or (None, None))]
        caches = []
        for s in sc:
            x = torch.tensor(rng.standard_normal((B, KH, cap, E)).astype(np.float32)) / (1.0 if s is None else s[None, :, None, None])
            x = x.to(torch.float8_e4m3fn)
            caches.append(x.to(DEV) if layout == "bhle" else x.transpose(1, 2).contiguous().to(DEV).transpose(1, 2))
        _INPUTS[key] = (q, *caches, *(None if s is None else s.to(DEV) for s in sc))
    return _INPUTS[key]


def _deq(cache, scale):
    """the cache as fp64 values: code value x the scale of its KV head"""
    x = VALUE[cache.view(torch.uint8).cpu().numpy()]
    return x if scale is None else x * scale.double().cpu().numpy()[None, :, None, None]


def _judge(name, dt, o, lse, o_ref, lse_ref, **case):
    """o per sequence under the type's gate, lse under the "f32" gate; both ratios go to the error log before anything is asserted"""
    assert np.isfinite(o_ref).all()
    got, dead = _f64(lse), lse_ref == NINF
    record_error("decode_attn_fp8", dict(name=name, dt=dt, o_ratio=max(_ratio(_f64(o[b]), o_ref[b], dt) for b in range(o_ref.shape[0])),
                                         lse_ratio=_ratio(got[~dead], lse_ref[~dead], "f32"), **case))
    for b in range(o_ref.shape[0]):
        assert_close(f"{name} o[{b}]", o[b], o_ref[b], dt, floor=not o_ref[b].any())
    assert (got[dead] == NINF).all(), f"{name}: lse of a row without a key or a sink"
    if (~dead).any():
        assert_close(f"{name} lse", got[~dead], lse_ref[~dead], "f32")


@pytest.mark.parametrize("E,dt,G,QL,cap,lens,splits,window,sinks,layout,scales", GRID,
                         ids=[f"E{c[0]}-{c[1]}-G{c[2]}-QL{c[3]}-L{'_'.join(map(str, c[5]))}-s{c[6]}-w{c[7]}-{'sink' if c[8] else 'nosink'}-{c[9]}-"
                              f"{'scaled' if c[10] else 'unscaled'}" for c in GRID])
def test_parity_against_fp64_on_the_dequantised_cache_with_the_nan_code_in_every_unseen_row(pkg, E, dt, G, QL, cap, lens, splits, window, sinks,
                                                                                            layout, scales):
    q, k0, v0, ks, vs = _inputs(E, dt, G, QL, layout, cap, scales)
    sk = None if sinks is None else np.resize(np.array(sinks), KH * G)
    k, v = k0.clone(), v0.clone()                        # clone keeps the strides of a transposed view
    assert k.stride() == k0.stride() and v.stride() == v0.stride()
    for b, n in enumerate(lens):
        first = 0 if window is None else max(0, n - QL - window)
        for c in (k.view(torch.uint8), v.view(torch.uint8)):
            c[b, :, :first], c[b, :, n:] = 0x7F, 0x7F
    o, lse = pkg.decode_attention_fp8(q, k, v, torch.tensor(lens, dtype=torch.int32, device=DEV), k_scale=ks, v_scale=vs, window_left=window,
                                      sinks=None if sk is None else torch.tensor(sk, dtype=torch.float32, device=DEV),
                                      num_splits=splits, return_lse=True)
    o_ref, lse_ref = ref_decode(_f64(q), _deq(k, ks), _deq(v, vs), lens, window, sk)         # the reference reads the poisoned caches too
    _judge("parity", dt, o, lse, o_ref, lse_ref, E=E, G=G, QL=QL, cap=cap, splits=splits)


@pytest.mark.parametrize("dt", ("f16", "bf16"))
@pytest.mark.parametrize("E", (64, 128))
def test_every_finite_code_converts_exactly_in_both_operands(pkg, E, dt):
    """Sequence b sees the one key b (window 0): its K row holds finite code number b in every column, its V row code number (b + e) mod
    254 in column e, and the query of head h is 1.0 in column 7 h mod E.  So o is V's row and lse the K code's value times 1 / sqrt(E),
    bit for bit.  The expectation adds +0.0: the accumulators start at +0, so the code -0 arrives as +0 like any sum that is zero."""
    n, T = len(FINITE), TORCH_DT[dt]
    k = torch.full((n, 1, n, E), 0x7F, dtype=torch.uint8)
    v = k.clone()
    idx = torch.arange(n)
    k[idx, 0, idx] = torch.tensor(FINITE)[:, None].expand(n, E)
    v[idx, 0, idx] = torch.tensor(FINITE[(np.arange(n)[:, None] + np.arange(E)[None, :]) % n])
    q = torch.zeros(n, 16, 1, E, dtype=T)
    q[:, idx[:16], 0, (7 * idx[:16]) % E] = 1.0
    o, lse = pkg.decode_attention_fp8(q.to(DEV), k.to(DEV).view(torch.float8_e4m3fn), v.to(DEV), torch.arange(1, n + 1, dtype=torch.int32, device=DEV),
                                      window_left=0, num_splits=1, return_lse=True)
    o_want = (torch.tensor(VALUE)[v[idx, 0, idx].long()] + 0.0).to(T)[:, None, None, :].expand(n, 16, 1, E)
    scale = torch.tensor(1.0 / np.sqrt(E), dtype=torch.float32)
    lse_want = ((torch.tensor(VALUE[FINITE]).float() + 0.0) * scale)[:, None, None].expand(n, 16, 1)
    assert torch.equal(o.cpu().view(torch.int16), o_want.contiguous().view(torch.int16))
    assert torch.equal(lse.cpu().view(torch.int32), lse_want.contiguous().view(torch.int32))


@pytest.mark.parametrize("E", (64, 128))
def test_a_sequences_bits_do_not_depend_on_the_batch(pkg, E):
    q, k, v, ks, vs = _inputs(E, "bf16", 8, 2, "blhe", CAP, SCALES[1])
    lens = torch.tensor((129, 33, CAP), dtype=torch.int32, device=DEV)
    kw = dict(k_scale=ks, v_scale=vs, window_left=128, sinks=torch.linspace(-1, 1, 16, device=DEV), num_splits=3, return_lse=True)
    o, lse = pkg.decode_attention_fp8(q, k, v, lens, **kw)
    for b in range(B):
        ob, lb = pkg.decode_attention_fp8(q[b:b + 1], k[b:b + 1], v[b:b + 1], lens[b:b + 1], **kw)
        assert torch.equal(ob[0], o[b]) and torch.equal(lb[0], lse[b]), b


def test_a_captured_call_follows_seqlens_and_the_cache(pkg):
    E, dt, G, QL = 64, "bf16", 8, 1
    q, k0, v0, ks, vs = _inputs(E, dt, G, QL, "bhle", CAP, SCALES[1])
    k, v = k0.clone(), v0.clone()
    lens = torch.tensor((127, 0, 31), dtype=torch.int32, device=DEV)
    splits, nbytes = pkg.decode_attention_fp8_plan(q, k, v, num_splits=3)
    assert (splits, nbytes) == pkg.decode_attention_plan(q, torch.empty_like(k, dtype=q.dtype), torch.empty_like(v, dtype=q.dtype), num_splits=3) == (3, 4 * B * KH * G * QL * 3 * (E + 2))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    o, lse = torch.empty_like(q), torch.empty(q.shape[:3], dtype=torch.float32, device=DEV)
    call = lambda o, lse: pkg.decode_attention_fp8_into(o, lse, q, k, v, lens, k_scale=ks, v_scale=vs, num_splits=3, workspace=ws)
    call(o, lse)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(o, lse)
    for step in range(3):                                # a decode step: one more row in each cache, every length advances
        for b in range(B):
            k.view(torch.uint8)[b, :, int(lens[b])], v.view(torch.uint8)[b, :, int(lens[b])] = 0x34 + step, 0xB0 + b
        lens += 1
        graph.replay()
        torch.cuda.synchronize()
        o_ref, lse_ref = ref_decode(_f64(q), _deq(k, ks), _deq(v, vs), lens.tolist(), None, None)
        _judge(f"replay {step}", dt, o, lse, o_ref, lse_ref)
        eager = call(torch.empty_like(o), torch.empty_like(lse))
        assert torch.equal(eager[0], o) and torch.equal(eager[1], lse), step
