"""GPU tests of prefill attention over a paged FP8 (E4M3) KV cache (include/nnop_hip_paged_prefill_fp8.h).  The reference is the thirteenth
library's test's plain fp64 softmax per row over the keys the row sees, on the codes gathered through the block table and DEQUANTISED
(code value x scale) and on the rounded q, so it holds no quantisation error and util.py's gates apply as they stand.  Without scales
every case also asks for the bits of paged_prefill_attention on the same pools cast to q's type: the codes are expanded at staging and
everything behind that is shared.  Shapes are that test's: new tokens at the edges of a row block of TB = 128 / G tokens, prefixes at
the edges of a 16-key block and of a 32-key tile, one of 130 or 257 in every case so that the second K/V image is refilled, pages of 16,
64 and 128.  Pools are the paged FP8 decode test's: live pages from a seeded permutation of a larger pool, one poison page, and the NaN
code 0x7F in every pool row that no query of its sequence sees.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

from test_zzzzzzzzzzzz_decode_attn_gpu import _f64
from test_zzzzzzzzzzzzz_decode_attn_fp8_gpu import SCALES, VALUE, _deq
from test_zzzzzzzzzzzzzz_paged_attn_gpu import _gather
from test_zzzzzzzzzzzzzzz_paged_prefill_gpu import B, CAP, KH, LAYOUTS, NEWS, PAGES, PREFIXES, ROWS, SINKS, WINDOWS, _judge, ref_prefill
from util import TORCH_DT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F8 = torch.float8_e4m3fn

# every (E, type, G) once, the other axes cycling: 16 cases of (E, dt, G, news index per sequence, prefix per sequence, window, sinks,
# layout, page, scales); sequence 0 stands behind 130 or 257 keys; then a sequence with fewer keys than new tokens
GRID = [(E, dt, G, tuple((5 * n + 7 * b) % 6 for b in range(B)), (PREFIXES[8 + n % 2],) + tuple(PREFIXES[(3 * n + 7 * b) % 10] for b in range(1, B)),
         WINDOWS[(n + n // 4) % 4], SINKS[(n // 2) % 2], LAYOUTS[(n // 3) % 2], PAGES[(n + n // 8) % 3], SCALES[(n + n // 2) % 2])
        for n, (E, dt, G) in enumerate(itertools.product((64, 128), ("f16", "bf16"), (1, 5, 8, 16)))]
assert all({c[i] for c in GRID} == set(vals) for i, vals in ((5, WINDOWS), (6, SINKS), (7, LAYOUTS), (8, PAGES), (9, SCALES)))
assert {i for c in GRID for i in c[3]} == set(range(6)) and {x for c in GRID for x in c[4]} == set(PREFIXES)
assert {(c[0], c[9]) for c in GRID} == set(itertools.product((64, 128), SCALES)) and {(c[1], c[9]) for c in GRID} == set(itertools.product(("f16", "bf16"), SCALES))
GRID += [(128, "bf16", 8, (4, 1, 5, 2), (-9, 0, -40, 33), 40, SINKS[1], "plhe", 16, SCALES[1])]

_INPUTS = {}


def _inputs(E, dt, G, scales):
    """q for the most tokens a case has, the logical K and V codes [B, KH, CAP, E] (standard normal over the scale, cast to E4M3 on the
    CPU: scale 1 reaches the subnormal codes) as uint8, and the two scales; made once per key and left unchanged"""
    key = (E, dt, G, scales)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * E + G)
        q = torch.tensor(rng.standard_normal((B * (2 * ROWS + 3), KH * G, E)).astype(np.float32)).to(TORCH_DT[dt]).to(DEV)
        sc = [None if scales is None else torch.tensor(s, dtype=torch.float32) for s in (scales or (None, None))]
        codes = [(torch.tensor(rng.standard_normal((B, KH, CAP, E)).astype(np.float32)) / (1.0 if s is None else s[None, :, None, None]))
                 .to(F8).view(torch.uint8).to(DEV) for s in sc]
        _INPUTS[key] = (q, *codes, *(None if s is None else s.to(DEV) for s in sc))
    return _INPUTS[key]


def _paged(k, v, news, lens, window, page, layout, num_pages, seed):
    """the uint8 pools (0x7F wherever no query looks) and the table: the pages that hold a visible key of a sequence are the next ones of
    a seeded permutation of the pool, taken page index by page index over the sequences; every other entry names its last page"""
    E, max_pages = k.shape[3], CAP // page
    perm = np.random.default_rng(seed).permutation(num_pages)
    assert num_pages > B * max_pages
    pools = [torch.full((num_pages, KH, page, E) if layout == "phle" else (num_pages, page, KH, E), 0x7F, dtype=torch.uint8, device=DEV)
             for _ in range(2)]
    kp, vp = (p if layout == "phle" else p.transpose(1, 2) for p in pools)
    table, free = np.full((B, max_pages), perm[-1], dtype=np.int32), iter(perm[:-1])
    for n, b in itertools.product(range(max_pages), range(B)):
        first = 0 if window is None else max(0, max(lens[b] - news[b], 0) - window)
        r0, r1 = max(first, n * page), min(lens[b] if news[b] else 0, (n + 1) * page)
        if r0 < r1:
            pg = table[b, n] = int(next(free))
            kp[pg, :, r0 - n * page:r1 - n * page], vp[pg, :, r0 - n * page:r1 - n * page] = k[b, :, r0:r1], v[b, :, r0:r1]
    return kp, vp, torch.tensor(table, device=DEV)


def _case(E, dt, G, news, prefixes, window, sinks, layout, page, scales, seed=0, spare=5):
    lens = tuple(max(c + n, 0) for c, n in zip(prefixes, news))
    q, k, v, ks, vs = _inputs(E, dt, G, scales)
    kp, vp, table = _paged(k, v, news, lens, window, page, layout, B * CAP // page + spare, seed=seed + page + E)
    sk = None if sinks is None else torch.tensor(np.resize(np.array(sinks), KH * G), dtype=torch.float32, device=DEV)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    kw = dict(k_scale=ks, v_scale=vs, window_left=window, sinks=sk, return_lse=True)
    return q[:sum(news)], kp, vp, table, i32(np.cumsum((0,) + news)), i32(lens), kw, lens


def _ref(q, kp, vp, table, news, lens, kw):
    sk = kw.get("sinks")
    return ref_prefill(_f64(q), _deq(_gather(kp, table), kw["k_scale"]), _deq(_gather(vp, table), kw["v_scale"]), news, lens,
                       kw["window_left"], None if sk is None else _f64(sk))


@pytest.mark.parametrize("E,dt,G,news,prefixes,window,sinks,layout,page,scales", GRID,
                         ids=[f"E{c[0]}-{c[1]}-G{c[2]}-n{'_'.join(map(str, c[3]))}-c{'_'.join(map(str, c[4]))}-w{c[5]}-{'sink' if c[6] else 'nosink'}-"
                              f"{c[7]}-p{c[8]}-{'scaled' if c[9] else 'unscaled'}" for c in GRID])
def test_parity_against_fp64_and_the_16_bit_calls_bits_with_the_nan_code_in_every_unseen_row(pkg, E, dt, G, news, prefixes, window, sinks, layout,
                                                                                            page, scales):
    news = tuple(NEWS(ROWS // G)[i] for i in news)
    q, kp, vp, table, cu, seqlens, kw, lens = _case(E, dt, G, news, prefixes, window, sinks, layout, page, scales)
    assert pkg.paged_prefill_attention_fp8_plan(q, kp, vp, table) == 0
    o, lse = pkg.paged_prefill_attention_fp8(q, kp.view(F8), vp, table, cu, seqlens, **kw)                   # both accepted dtypes
    assert o.shape == q.shape and lse.shape == q.shape[:2]
    ref = _ref(q, kp, vp, table, news, lens, kw)
    assert ref[2].any() == any(c < 0 for c in prefixes)
    _judge("parity", dt, o, lse, ref, news, E=E, G=G, page=page, fp8=True)
    if scales is None:
        o16, lse16 = pkg.paged_prefill_attention(q, kp.view(F8).to(q.dtype), vp.view(F8).to(q.dtype), table, cu, seqlens, window_left=window,
                                                 sinks=kw["sinks"], return_lse=True)
        assert torch.equal(o, o16) and torch.equal(lse, lse16), "not the bits of paged_prefill_attention on the pools cast to q's type"


@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_every_code_converts_exactly(pkg, dt):
    """Two sequences of one token and one key each at E = 128: the V row of sequence b holds codes 128 b ... 128 b + 127, the two NaN
    codes replaced by 0, and its K row 1.0, so the softmax is the weight 1 and o is V's row, bit for bit.  The expectation adds +0.0:
    the accumulators start at +0, so the code -0 arrives as +0 like any sum that is zero."""
    T = TORCH_DT[dt]
    codes = torch.arange(256, dtype=torch.uint8)
    codes[codes & 0x7F == 0x7F] = 0
    kp, vp = (torch.full((2, 1, 16, 128), 0x7F, dtype=torch.uint8) for _ in range(2))
    kp[:, 0, 0], vp[:, 0, 0] = 0x38, codes.view(2, 128)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    o = pkg.paged_prefill_attention_fp8(torch.ones(2, 3, 128, dtype=T, device=DEV), kp.to(DEV), vp.to(DEV), i32([[0], [1]]), i32([0, 1, 2]), i32([1, 1]))
    want = (torch.tensor(VALUE)[codes.long()] + 0.0).to(T).view(2, 1, 128).expand(2, 3, 128)
    assert torch.equal(o.cpu().view(torch.int16), want.contiguous().view(torch.int16))


def test_the_bits_depend_neither_on_where_the_pages_lie_nor_on_the_batch_nor_on_the_run(pkg):
    news, prefixes = (35, 16, 1, 17), (130, 0, 257, 63)
    q, kp, vp, table, cu, seqlens, kw, lens = _case(64, "bf16", 8, news, prefixes, 128, SINKS[1], "plhe", 16, SCALES[1])
    o, lse = pkg.paged_prefill_attention_fp8(q, kp, vp, table, cu, seqlens, **kw)
    _, kp2, vp2, table2, *_ = _case(64, "bf16", 8, news, prefixes, 128, SINKS[1], "phle", 16, SCALES[1], seed=1, spare=47)   # the same keys elsewhere
    assert not torch.equal(table, table2)
    for pools in ((kp2, vp2, table2), (kp, vp, table)):                                                      # and the first call once more
        o2, lse2 = pkg.paged_prefill_attention_fp8(q, *pools, cu, seqlens, **kw)
        assert torch.equal(o2, o) and torch.equal(lse2, lse)
    for b in range(B):
        s = slice(int(cu[b]), int(cu[b + 1]))
        ob, lb = pkg.paged_prefill_attention_fp8(q[s], kp, vp, table[b:b + 1], cu[b:b + 2] - cu[b], seqlens[b:b + 1], **kw)
        assert torch.equal(ob, o[s]) and torch.equal(lb, lse[s]), b


def test_a_captured_call_follows_cu_seqlens_seqlens_the_table_the_pages_and_the_scales(pkg):
    E, dt, G, page, T = 64, "bf16", 8, 16, 70
    q, k, v, ks0, vs0 = _inputs(E, dt, G, SCALES[1])
    q, ks, vs = q[:T], ks0.clone(), vs0.clone()
    kp, vp, table = _paged(k, v, (1,) * B, (CAP,) * B, None, page, "plhe", B * CAP // page + 5, seed=3)   # every key of every sequence
    cu, seqlens = (torch.zeros(n, dtype=torch.int32, device=DEV) for n in (B + 1, B))
    o, lse = torch.empty_like(q), torch.empty(q.shape[:2], dtype=torch.float32, device=DEV)
    kw = dict(k_scale=ks, v_scale=vs, window_left=100, sinks=None)
    call = lambda o, lse: pkg.paged_prefill_attention_fp8_into(o, lse, q, kp, vp, table, cu, seqlens, k_scale=ks, v_scale=vs, window_left=100)
    call(o, lse)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(o, lse)
    for step, (news, lens) in enumerate((((20, 5, 0, 45), (150, 5, 64, 45)), ((0, 33, 17, 20), (9, 300, 17, 147)), ((16, 17, 18, 19), (16, 130, 257, 19)))):
        cu.copy_(torch.tensor(np.cumsum((0,) + news), dtype=torch.int32))
        seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
        a, c = (int(x) for x in table[1, step:step + 2])  # two pages of sequence 1 change places in the pool
        for pool in (kp, vp):
            pool[[a, c]] = pool[[c, a]]
        table[1, step], table[1, step + 1] = c, a
        (ks, vs)[step % 2][step % KH] *= 1.25            # and one scale value changes
        graph.replay()
        torch.cuda.synchronize()
        _judge(f"replay {step}", dt, o, lse, _ref(q, kp, vp, table, news, lens, kw), news, fp8=True)
        eager = call(torch.empty_like(o), torch.empty_like(lse))
        assert torch.equal(eager[0], o) and torch.equal(eager[1], lse), step
