"""GPU tests of prefill attention over a paged KV cache (include/nnop_hip_paged_prefill.h).  The reference is a plain fp64 softmax per row
over the keys the row sees, on the keys gathered through the block table.  New tokens per sequence at the edges of a row block of
TB = 128 / G tokens (0, 1, TB - 1, TB, TB + 1, 2 TB + 3), cached prefixes at the edges of a 16-key block and of a 32-key tile and long
enough (130, 257) for every block to run at least three tiles, so the second K/V image is refilled; pages of 16, 64 and 128 (a tile
spans two pages, half a page, a quarter).  Live pages are drawn from a seeded permutation of a larger pool; every table entry without a
visible key names one poison page, and every pool row that no query of its sequence sees holds NaN in K and V.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from test_zzzzzzzzzzzz_decode_attn_gpu import _f64, _ratio
from util import TORCH_DT, assert_close, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = ge.load_package()._lib_paged_prefill.BLOCK_ROWS
CAP, KH, B = 640, 2, 4
NEWS = lambda TB: (0, 1, TB - 1, TB, TB + 1, 2 * TB + 3)
PREFIXES = (0, 1, 15, 16, 17, 63, 64, 65, 130, 257)
WINDOWS = (None, 0, 40, 128)
SINKS = (None, (-np.inf, 0.7, 30.0))
LAYOUTS = ("phle", "plhe")                               # [P, KH, page, E]; [P, page, KH, E] passed transposed
PAGES = (16, 64, 128)
NINF = -np.inf

# every (E, type, G) twice, the other axes cycling: 32 cases of (E, dt, G, news index per sequence, prefix per sequence, window, sinks,
# layout, page); then a sequence with fewer keys than new tokens (its first rows stand below 0) and a call without a token
GRID = [(E, dt, G, tuple((5 * n + 7 * b) % 6 for b in range(B)), tuple(PREFIXES[(3 * n + 7 * b) % 10] for b in range(B)), WINDOWS[(n + n // 4) % 4],
         SINKS[(n // 2) % 2], LAYOUTS[(n // 3) % 2], PAGES[(n + n // 8) % 3])
        for n, (E, dt, G, _) in enumerate(itertools.product((64, 128), ("f16", "bf16"), (1, 5, 8, 16), range(2)))]
assert all({c[i] for c in GRID} == set(vals) for i, vals in ((5, WINDOWS), (6, SINKS), (7, LAYOUTS), (8, PAGES)))
assert {i for c in GRID for i in c[3]} == set(range(6)) and {x for c in GRID for x in c[4]} == set(PREFIXES)
assert {(c[0], c[8]) for c in GRID} == set(itertools.product((64, 128), PAGES))
GRID += [(128, "bf16", 8, (4, 1, 5, 2), (-9, 0, -40, 33), 40, SINKS[1], "plhe", 16), (64, "f16", 5, (0, 0, 0, 0), (0, 1, 16, 257), None, None, "phle", 64)]

_INPUTS = {}


def _inputs(E, dt, G):
    """q for the most tokens a case has and the logical keys and values [B, KH, CAP, E], made once per key and left unchanged"""
    if (E, dt, G) not in _INPUTS:
        rng = np.random.default_rng(1000 * E + G)
        mk = lambda *s: torch.tensor(rng.standard_normal(s).astype(np.float32)).to(TORCH_DT[dt]).to(DEV)
        _INPUTS[E, dt, G] = (mk(B * (2 * ROWS + 3), KH * G, E), mk(B, KH, CAP, E), mk(B, KH, CAP, E))
    return _INPUTS[E, dt, G]


def _paged(k, v, news, lens, window, page, layout, num_pages, seed):
    """test_zzzzzzzzzzzzzz_paged_attn_gpu's pools with a QL per sequence: NaN wherever no query looks, the pages that hold a visible key
    drawn from a seeded permutation of the pool sequence by sequence in turn, every other table entry the permutation's last page"""
    E, max_pages = k.shape[3], CAP // page
    perm = np.random.default_rng(seed).permutation(num_pages)
    assert num_pages > B * max_pages
    pools = [torch.full((num_pages, KH, page, E) if layout == "phle" else (num_pages, page, KH, E), float("nan"), dtype=k.dtype, device=DEV)
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


def _gather(pool, table):
    g = pool[table.long()]                               # [B, max_pages, KH, page, E]
    return _f64(g.permute(0, 2, 1, 3, 4).reshape(g.shape[0], g.shape[2], -1, g.shape[4]))


def ref_prefill(q, k, v, news, lens, window, sinks):
    """fp64: query i of sequence b stands at p = lens[b] - news[b] + i and sees max(0, p - window) ... p; a row without a key is 0, lse its sink"""
    (T, QH, E), G = q.shape, q.shape[1] // k.shape[1]
    o, lse, dead, t0 = np.zeros_like(q), np.full((T, QH), NINF), np.zeros((T, QH), bool), np.cumsum((0,) + tuple(news))
    for b, h in itertools.product(range(len(news)), range(QH)):
        for i in range(news[b]):
            p, t = lens[b] - news[b] + i, t0[b] + i
            js = np.arange(0 if window is None else max(0, p - window), p + 1)
            cols = np.append(k[b, h // G, js] @ q[t, h] / np.sqrt(E), [] if sinks is None else sinks[h])
            dead[t, h] = js.size == 0
            if cols.size and cols.max() > NINF:
                w = np.exp(cols - cols.max())
                lse[t, h], o[t, h] = cols.max() + np.log(w.sum()), (w[:js.size] / w.sum()) @ v[b, h // G, js]
    return o, lse, dead


def _judge(name, dt, o, lse, ref, news, **case):
    """o per sequence under the type's gate, lse under the "f32" gate and exactly where a row saw no key; the ratios go to the error log first"""
    (o_ref, lse_ref, dead), t0, got = ref, np.cumsum((0,) + tuple(news)), _f64(lse)
    seqs = [slice(t0[b], t0[b + 1]) for b in range(len(news)) if news[b]]
    assert np.isfinite(o_ref).all() and not torch.isnan(o).any()
    record_error("paged_prefill", dict(name=name, dt=dt, o_ratio=max([_ratio(_f64(o[s]), o_ref[s], dt) for s in seqs], default=0.0),
                                       lse_ratio=_ratio(got[~dead], lse_ref[~dead], "f32"), **case))
    for s in seqs:
        assert_close(f"{name} o[{s}]", o[s], o_ref[s], dt, floor=not o_ref[s].any())
    assert (got[dead] == lse_ref[dead].astype(np.float32)).all() and not _f64(o)[dead].any(), f"{name}: a row without a key"
    if (~dead).any():
        assert_close(f"{name} lse", got[~dead], lse_ref[~dead], "f32")


def _case(E, dt, G, news, prefixes, window, sinks, layout, page, seed=0, spare=5):
    lens = tuple(max(c + n, 0) for c, n in zip(prefixes, news))
    q, k, v = _inputs(E, dt, G)
    kp, vp, table = _paged(k, v, news, lens, window, page, layout, B * CAP // page + spare, seed=seed + page + E)
    sk = None if sinks is None else torch.tensor(np.resize(np.array(sinks), KH * G), dtype=torch.float32, device=DEV)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    return q[:sum(news)], kp, vp, table, i32(np.cumsum((0,) + news)), i32(lens), dict(window_left=window, sinks=sk, return_lse=True), lens


@pytest.mark.parametrize("E,dt,G,news,prefixes,window,sinks,layout,page", GRID,
                         ids=[f"E{c[0]}-{c[1]}-G{c[2]}-n{'_'.join(map(str, c[3]))}-c{'_'.join(map(str, c[4]))}-w{c[5]}-{'sink' if c[6] else 'nosink'}-"
                              f"{c[7]}-p{c[8]}" for c in GRID])
def test_parity_against_fp64_with_nan_in_every_unseen_row(pkg, E, dt, G, news, prefixes, window, sinks, layout, page):
    news = tuple(NEWS(ROWS // G)[i] for i in news)
    q, kp, vp, table, cu, seqlens, kw, lens = _case(E, dt, G, news, prefixes, window, sinks, layout, page)
    assert pkg.paged_prefill_attention_plan(q, kp, vp, table) == 0
    o, lse = pkg.paged_prefill_attention(q, kp, vp, table, cu, seqlens, **kw)
    assert o.shape == q.shape and lse.shape == q.shape[:2]
    ref = ref_prefill(_f64(q), _gather(kp, table), _gather(vp, table), news, lens, window, None if sinks is None else _f64(kw["sinks"]))
    assert ref[2].any() == any(c < 0 for c in prefixes)
    _judge("parity", dt, o, lse, ref, news, E=E, G=G, page=page)


def test_the_bits_depend_neither_on_where_the_pages_lie_nor_on_the_batch_nor_on_the_run(pkg):
    news, prefixes = (35, 16, 1, 17), (130, 0, 257, 63)
    q, kp, vp, table, cu, seqlens, kw, lens = _case(64, "bf16", 8, news, prefixes, 128, SINKS[1], "plhe", 16)
    o, lse = pkg.paged_prefill_attention(q, kp, vp, table, cu, seqlens, **kw)
    _, kp2, vp2, table2, *_ = _case(64, "bf16", 8, news, prefixes, 128, SINKS[1], "phle", 16, seed=1, spare=47)   # the same keys elsewhere
    assert not torch.equal(table, table2)
    for pools in ((kp2, vp2, table2), (kp, vp, table)):                                                      # and the first call once more
        o2, lse2 = pkg.paged_prefill_attention(q, *pools, cu, seqlens, **kw)
        assert torch.equal(o2, o) and torch.equal(lse2, lse)
    for b in range(B):
        s = slice(int(cu[b]), int(cu[b + 1]))
        ob, lb = pkg.paged_prefill_attention(q[s], kp, vp, table[b:b + 1], cu[b:b + 2] - cu[b], seqlens[b:b + 1], **kw)
        assert torch.equal(ob, o[s]) and torch.equal(lb, lse[s]), b


def test_a_captured_call_follows_cu_seqlens_seqlens_the_table_and_the_pages(pkg):
    E, dt, G, page, T = 64, "bf16", 8, 16, 70
    q, k, v = _inputs(E, dt, G)
    q = q[:T]
    kp, vp, table = _paged(k, v, (1,) * B, (CAP,) * B, None, page, "plhe", B * CAP // page + 5, seed=3)   # every key of every sequence
    cu, seqlens = (torch.zeros(n, dtype=torch.int32, device=DEV) for n in (B + 1, B))
    ws = torch.empty(pkg.paged_prefill_attention_plan(q, kp, vp, table), dtype=torch.uint8, device=DEV)
    o, lse = torch.empty_like(q), torch.empty(q.shape[:2], dtype=torch.float32, device=DEV)
    call = lambda o, lse: pkg.paged_prefill_attention_into(o, lse, q, kp, vp, table, cu, seqlens, window_left=100, workspace=ws)
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
        graph.replay()
        torch.cuda.synchronize()
        _judge(f"replay {step}", dt, o, lse, ref_prefill(_f64(q), _gather(kp, table), _gather(vp, table), news, lens, 100, None), news)
        eager = call(torch.empty_like(o), torch.empty_like(lse))
        assert torch.equal(eager[0], o) and torch.equal(eager[1], lse), step
