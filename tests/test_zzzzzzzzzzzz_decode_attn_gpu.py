"""GPU tests of decode attention over a KV cache (include/nnop_hip_decode_attn.h).  The reference is the plain fp64 softmax over the keys
a query sees, written below from the header's rule.  Shapes: capacity 300 = nine tiles of 32 keys and a ragged tenth; lengths at a tile
edge, at one round of the four waves (128) and one beside each, 0, 1 (below QL = 2) and the capacity, each with each of 1, 3 and 7
splits (7 leaves chunks without a tile at short lengths); (G, QL) with 1, 5, 8 and 16 rows of the 16-wide operand.  A wave's ring of two
tiles is refilled only from 9 tiles per chunk on and wraps twice from 17, so the LONG cases have a capacity of 1100 = 35 tiles: 35 per
chunk at one split (a wave consumes 9: five loop iterations, the last with one slot), 12 at three; behind a window of 900 29 live tiles, 10 per
chunk at three splits.
In every parity case every cache row that no query of its sequence sees holds NaN in K and in V.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

from util import ATOL_FRAC, RTOL, TORCH_DT, assert_close, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP, LONG_CAP, KH, B = 300, 1100, 2, 3
LENS = (0, 1, 31, 32, 33, 127, 128, 129, CAP)
ROWS = ((1, 1), (5, 1), (8, 1), (16, 1), (8, 2))         # (G, QL)
WINDOWS = (None, 0, 5, 40, 128)
SPLITS = (1, 3, 7)
SINKS = (None, (-np.inf, 0.7, 30.0))
LAYOUTS = ("bhle", "blhe")
PER_COMBO = 6
NINF = -np.inf


def _grid():
    """every (E, type, (G, QL)) six times, the other axes cycling -- the splits shifted by one every nine cases, so that every length
    meets every split count: 120 cases; then the 8 LONG ones, (E, splits, window) in full, the rest alternating"""
    cases = []
    for n, (E, dt, (G, QL), r) in enumerate(itertools.product((64, 128), ("f16", "bf16"), ROWS, range(PER_COMBO))):
        lens = (LENS[n % 9], LENS[(2 * n + 3) % 9], LENS[(4 * n + 7) % 9])
        cases.append((E, dt, G, QL, CAP, lens, SPLITS[(n + n // 9) % 3], WINDOWS[(n // 3) % 5], SINKS[(n // 2) % 2], LAYOUTS[(n // 5) % 2]))
    for n, (E, splits, window) in enumerate(itertools.product((64, 128), (1, 3), (None, 900))):
        cases.append((E, ("bf16", "f16")[(n + n // 2) % 2], 8, 1 + n // 2 % 2, LONG_CAP, (LONG_CAP, 577, 289), splits, window, SINKS[(n + n // 4) % 2],
                      LAYOUTS[n // 2 % 2]))
    return cases


GRID = _grid()
SHORT = [c for c in GRID if c[4] == CAP]
assert all({c[i] for c in SHORT} == set(vals) for i, vals in ((6, SPLITS), (7, WINDOWS), (8, SINKS), (9, LAYOUTS)))
assert {(n, c[6]) for c in SHORT for n in c[5]} == set(itertools.product(LENS, SPLITS)) and any(c[3] == 2 and 1 in c[5] for c in SHORT)

_INPUTS = {}


def _inputs(E, dt, G, QL, layout, cap=CAP):
    """q and the two caches, made once per key and left unchanged (tests clone what they overwrite)"""
    key = (E, dt, G, QL, layout, cap)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * E + 10 * G + QL)
        mk = lambda *s: torch.tensor(rng.standard_normal(s).astype(np.float32)).to(TORCH_DT[dt]).to(DEV)
        q = mk(B, KH * G, QL, E)
        k, v = (mk(B, KH, cap, E) if layout == "bhle" else mk(B, cap, KH, E).transpose(1, 2) for _ in range(2))
        _INPUTS[key] = (q, k, v)
    return _INPUTS[key]


def _f64(t):
    return t.detach().double().cpu().numpy()


def ref_decode(q, k, v, lens, window, sinks):
    """fp64: query i of sequence b stands at p = lens[b] - QL + i and sees max(0, p - window) ... p; a row without a key is 0, lse its sink"""
    (Bq, QH, QL, E), G = q.shape, q.shape[1] // k.shape[1]
    o, lse = np.zeros_like(q), np.full(q.shape[:3], NINF)
    for b, h, i in itertools.product(range(Bq), range(QH), range(QL)):
        p = int(lens[b]) - QL + i
        js = np.arange(0 if window is None else max(0, p - window), p + 1)
        x = k[b, h // G, js] @ q[b, h, i] / np.sqrt(E)
        cols = x if sinks is None else np.append(x, sinks[h])
        if cols.size and cols.max() > NINF:
            w = np.exp(cols - cols.max())
            lse[b, h, i] = cols.max() + np.log(w.sum())
            o[b, h, i] = (w[:js.size] / w.sum()) @ v[b, h // G, js]
    return o, lse


def _poison(k, v, lens, QL, window):
    """copies of the caches in which every row that no query of its sequence sees holds NaN"""
    k, v = k.clone(), v.clone()                          # clone keeps the strides of a transposed view
    for b, n in enumerate(lens):
        first = 0 if window is None else max(0, n - QL - window)
        k[b, :, :first], v[b, :, :first], k[b, :, n:], v[b, :, n:] = (float("nan"),) * 4
    return k, v


def _ratio(got, ref, dt):
    """worst |got - ref| over util.assert_close's gate for the type (scale 1, no floor); 0 where there is nothing to judge"""
    tol = ATOL_FRAC[dt] * np.abs(ref).max(initial=0.0) + RTOL[dt] * np.abs(ref)
    return float((np.abs(got - ref)[tol > 0] / tol[tol > 0]).max(initial=0.0))


def _judge(name, dt, o, lse, o_ref, lse_ref, **case):
    """o per sequence under the type's gate, lse under the "f32" gate; both ratios go to the error log before anything is asserted"""
    got, dead = _f64(lse), lse_ref == NINF
    record_error("decode_attn", dict(name=name, dt=dt, o_ratio=max(_ratio(_f64(o[b]), o_ref[b], dt) for b in range(o_ref.shape[0])),
                                     lse_ratio=_ratio(got[~dead], lse_ref[~dead], "f32"), **case))
    for b in range(o_ref.shape[0]):
        assert_close(f"{name} o[{b}]", o[b], o_ref[b], dt, floor=not o_ref[b].any())
    assert (got[dead] == NINF).all(), f"{name}: lse of a row without a key or a sink"
    if (~dead).any():
        assert_close(f"{name} lse", got[~dead], lse_ref[~dead], "f32")


@pytest.mark.parametrize("E,dt,G,QL,cap,lens,splits,window,sinks,layout", GRID,
                         ids=[f"E{c[0]}-{c[1]}-G{c[2]}-QL{c[3]}-L{'_'.join(map(str, c[5]))}-s{c[6]}-w{c[7]}-{'sink' if c[8] else 'nosink'}-{c[9]}"
                              for c in GRID])
def test_parity_against_fp64_with_nan_in_every_unseen_row(pkg, E, dt, G, QL, cap, lens, splits, window, sinks, layout):
    q, k0, v0 = _inputs(E, dt, G, QL, layout, cap)
    sk = None if sinks is None else np.resize(np.array(sinks), KH * G)
    k, v = _poison(k0, v0, lens, QL, window)
    assert k.stride() == k0.stride() and v.stride() == v0.stride()
    o, lse = pkg.decode_attention(q, k, v, torch.tensor(lens, dtype=torch.int32, device=DEV), window_left=window,
                                  sinks=None if sk is None else torch.tensor(sk, dtype=torch.float32, device=DEV),
                                  num_splits=splits, return_lse=True)
    o_ref, lse_ref = ref_decode(_f64(q), _f64(k), _f64(v), lens, window, sk)      # the reference reads the poisoned caches too
    assert np.isfinite(o_ref).all()
    _judge("parity", dt, o, lse, o_ref, lse_ref, E=E, G=G, QL=QL, cap=cap, splits=splits)


@pytest.mark.parametrize("E", (64, 128))
def test_a_sequences_bits_do_not_depend_on_the_batch(pkg, E):
    q, k, v = _inputs(E, "bf16", 8, 2, "blhe")
    lens = torch.tensor((129, 33, CAP), dtype=torch.int32, device=DEV)
    sinks = torch.linspace(-1, 1, 16, device=DEV)
    o, lse = pkg.decode_attention(q, k, v, lens, window_left=128, sinks=sinks, num_splits=3, return_lse=True)
    for b in range(B):
        ob, lb = pkg.decode_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], lens[b:b + 1], window_left=128, sinks=sinks, num_splits=3,
                                      return_lse=True)
        assert torch.equal(ob[0], o[b]) and torch.equal(lb[0], lse[b]), b


def test_a_captured_call_follows_seqlens_and_the_cache(pkg):
    E, dt, G, QL = 64, "bf16", 8, 1
    q, k0, v0 = _inputs(E, dt, G, QL, "bhle")
    k, v = k0.clone(), v0.clone()
    lens = torch.tensor((127, 0, 31), dtype=torch.int32, device=DEV)
    splits, nbytes = pkg.decode_attention_plan(q, k, v, num_splits=3)
    assert splits == 3 and nbytes == 4 * B * KH * G * QL * 3 * (E + 2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    o, lse = torch.empty_like(q), torch.empty(q.shape[:3], dtype=torch.float32, device=DEV)
    call = lambda o, lse: pkg.decode_attention_into(o, lse, q, k, v, lens, num_splits=3, workspace=ws)
    call(o, lse)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(o, lse)
    for step in range(3):                                # a decode step: one more row in each cache, every length advances
        for b in range(B):
            k[b, :, int(lens[b])], v[b, :, int(lens[b])] = 0.5 * (step + 1), -0.25 * (b + 1)
        lens += 1
        graph.replay()
        torch.cuda.synchronize()
        o_ref, lse_ref = ref_decode(_f64(q), _f64(k), _f64(v), lens.tolist(), None, None)
        _judge(f"replay {step}", dt, o, lse, o_ref, lse_ref)
        eager = call(torch.empty_like(o), torch.empty_like(lse))
        assert torch.equal(eager[0], o) and torch.equal(eager[1], lse), step


@pytest.mark.parametrize("E", (64, 128))
def test_flash_attention_with_a_length_mask_agrees(pkg, E):
    dt, G = "f16", 8
    q, k, v = _inputs(E, dt, G, 1, "bhle")
    lens = (129, 1, CAP)
    o = pkg.decode_attention(q, k, v, torch.tensor(lens, dtype=torch.int32, device=DEV))
    mask = torch.arange(CAP, device=DEV)[None, :] < torch.tensor(lens, device=DEV)[:, None]
    o_fa = pkg.flash_attention(q, k, v, causal=False, kpad_mask=mask)
    o_ref, _ = ref_decode(_f64(q), _f64(k), _f64(v), lens, None, None)
    for b in range(B):
        assert_close(f"decode o[{b}]", o[b], o_ref[b], dt)
        assert_close(f"flash o[{b}]", o_fa[b], o_ref[b], dt)
