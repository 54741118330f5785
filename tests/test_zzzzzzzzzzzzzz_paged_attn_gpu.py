"""GPU tests of decode attention over a paged KV cache (include/nnop_hip_paged_attn.h).  The reference is the tenth library's test's plain
fp64 softmax over the keys a query sees, on the keys gathered through the block table; every case also asks for the bits of
decode_attention on that gathered cache at the same split count.  Shapes: 320 keys of table per sequence in pages of 16, 32 and 64 (a
tile of 32 keys spans two pages, is one page, is half a page); lengths at a page and a tile edge, at one round of the four waves and one
beside each, 0, 1 and the whole table; 1 / 3 / 7 splits.  A wave's ring of two tiles is refilled -- from table entries fetched a refill
earlier -- only from 9 tiles per chunk on, so the LONG cases have 1152 keys = 36 tiles, in pages of 16 and 128.
A sequence's live pages are drawn from a seeded permutation of a pool larger than the tables, so neighbouring keys lie in distant pages
and the sequences interleave; every table entry without a visible key names one poison page, and every pool row that no query of its
sequence sees -- the rest of a partly filled page, pages in front of the window, unowned pages, the poison page -- holds NaN in K and V.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

from test_zzzzzzzzzzzz_decode_attn_gpu import _f64, _ratio, ref_decode
from util import TORCH_DT, assert_close, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP, LONG_CAP, KH, B = 320, 1152, 2, 3
LENS = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, CAP)
ROWS = ((1, 1), (5, 1), (16, 1), (8, 2))                 # (G, QL)
WINDOWS = (None, 0, 40, 128)
SPLITS = (1, 3, 7)
SINKS = (None, (-np.inf, 0.7, 30.0))
LAYOUTS = ("phle", "plhe")                               # [P, KH, page, E]; [P, page, KH, E] passed transposed
PAGES = (16, 32, 64)
NINF = -np.inf

# every (E, type, (G, QL)) three times, the other axes cycling: 48 cases; then the 4 LONG ones
GRID = [(E, dt, G, QL, CAP, (LENS[n % 12], LENS[(5 * n + 3) % 12], LENS[(7 * n + 7) % 12]), SPLITS[(n + n // 9) % 3], WINDOWS[(n // 3) % 4],
         SINKS[(n // 2) % 2], LAYOUTS[(n // 5) % 2], PAGES[(n + n // 6) % 3])
        for n, (E, dt, (G, QL), _) in enumerate(itertools.product((64, 128), ("f16", "bf16"), ROWS, range(3)))]
assert all({c[i] for c in GRID} == set(vals) for i, vals in ((6, SPLITS), (7, WINDOWS), (8, SINKS), (9, LAYOUTS), (10, PAGES)))
assert {n for c in GRID for n in c[5]} == set(LENS) and {(c[0], c[10]) for c in GRID} == set(itertools.product((64, 128), PAGES))
GRID += [(E, ("bf16", "f16")[n % 2], 8, 1 + n % 2, LONG_CAP, (LONG_CAP, 577, 289), splits, window, SINKS[n % 2], LAYOUTS[n % 2], page)
         for n, (E, page, splits, window) in enumerate([(64, 16, 1, None), (64, 128, 2, 900), (128, 128, 1, None), (128, 16, 2, None)])]

_INPUTS = {}


def _inputs(E, dt, G, QL, cap):
    """q and the logical keys and values [B, KH, cap, E], made once per key and left unchanged"""
    key = (E, dt, G, QL, cap)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * E + 10 * G + QL)
        mk = lambda *s: torch.tensor(rng.standard_normal(s).astype(np.float32)).to(TORCH_DT[dt]).to(DEV)
        _INPUTS[key] = (mk(B, KH * G, QL, E), mk(B, KH, cap, E), mk(B, KH, cap, E))
    return _INPUTS[key]


def _paged(k, v, lens, QL, window, page, layout, num_pages, seed):
    """the pools (NaN wherever no query looks) and the table: the pages that hold a visible key of a sequence are the next ones of a
    seeded permutation of the pool, taken sequence by sequence in turn; every other entry names the permutation's last page"""
    cap, E = k.shape[2], k.shape[3]
    max_pages = cap // page
    perm = np.random.default_rng(seed).permutation(num_pages)
    assert num_pages > B * max_pages
    pools = [torch.full((num_pages, KH, page, E) if layout == "phle" else (num_pages, page, KH, E), float("nan"), dtype=k.dtype, device=DEV)
             for _ in range(2)]
    kp, vp = (p if layout == "phle" else p.transpose(1, 2) for p in pools)
    table, free = np.full((B, max_pages), perm[-1], dtype=np.int32), iter(perm[:-1])
    for n, b in itertools.product(range(max_pages), range(B)):   # page by page, so the sequences interleave in the permutation
        first = 0 if window is None else max(0, lens[b] - QL - window)
        r0, r1 = max(first, n * page), min(lens[b], (n + 1) * page)
        if r0 < r1:
            pg = table[b, n] = int(next(free))
            kp[pg, :, r0 - n * page:r1 - n * page], vp[pg, :, r0 - n * page:r1 - n * page] = k[b, :, r0:r1], v[b, :, r0:r1]
    return kp, vp, torch.tensor(table, device=DEV)


def _gather(pool, table):
    """the dense cache [B, KH, max_pages page, E] a table names"""
    g = pool[table.long()]                               # [B, max_pages, KH, page, E]
    return g.permute(0, 2, 1, 3, 4).reshape(g.shape[0], g.shape[2], -1, g.shape[4])


def _judge(name, dt, o, lse, o_ref, lse_ref, **case):
    """o per sequence under the type's gate, lse under the "f32" gate; both ratios go to the error log before anything is asserted"""
    assert np.isfinite(o_ref).all()
    got, dead = _f64(lse), lse_ref == NINF
    record_error("paged_attn", dict(name=name, dt=dt, o_ratio=max(_ratio(_f64(o[b]), o_ref[b], dt) for b in range(o_ref.shape[0])),
                                    lse_ratio=_ratio(got[~dead], lse_ref[~dead], "f32"), **case))
    for b in range(o_ref.shape[0]):
        assert_close(f"{name} o[{b}]", o[b], o_ref[b], dt, floor=not o_ref[b].any())
    assert (got[dead] == NINF).all(), f"{name}: lse of a row without a key or a sink"
    if (~dead).any():
        assert_close(f"{name} lse", got[~dead], lse_ref[~dead], "f32")


@pytest.mark.parametrize("E,dt,G,QL,cap,lens,splits,window,sinks,layout,page", GRID,
                         ids=[f"E{c[0]}-{c[1]}-G{c[2]}-QL{c[3]}-L{'_'.join(map(str, c[5]))}-s{c[6]}-w{c[7]}-{'sink' if c[8] else 'nosink'}-{c[9]}-"
                              f"p{c[10]}" for c in GRID])
def test_parity_against_fp64_and_the_dense_calls_bits_with_nan_in_every_unseen_row(pkg, E, dt, G, QL, cap, lens, splits, window, sinks, layout, page):
    q, k, v = _inputs(E, dt, G, QL, cap)
    kp, vp, table = _paged(k, v, lens, QL, window, page, layout, B * cap // page + 5, seed=page + E)
    assert kp.stride() != kp.contiguous().stride() or layout == "phle"
    sk = None if sinks is None else torch.tensor(np.resize(np.array(sinks), KH * G), dtype=torch.float32, device=DEV)
    kw = dict(window_left=window, sinks=sk, num_splits=splits, return_lse=True)
    seqlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o, lse = pkg.paged_decode_attention(q, kp, vp, table, seqlens, **kw)
    kd, vd = _gather(kp, table), _gather(vp, table)      # NaN in every row no query sees: the reference and the dense call read it too
    o_ref, lse_ref = ref_decode(_f64(q), _f64(kd), _f64(vd), lens, window, None if sk is None else _f64(sk))
    _judge("parity", dt, o, lse, o_ref, lse_ref, E=E, G=G, QL=QL, cap=cap, splits=splits, page=page)
    od, lsed = pkg.decode_attention(q, kd, vd, seqlens, **kw)
    assert torch.equal(o, od) and torch.equal(lse, lsed), "not the bits of decode_attention on the gathered cache"


@pytest.mark.parametrize("E", (64, 128))
def test_the_bits_depend_neither_on_where_the_pages_lie_nor_on_the_batch(pkg, E):
    q, k, v = _inputs(E, "bf16", 8, 2, CAP)
    lens, page = (129, 33, CAP), 16
    seqlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kw = dict(window_left=128, sinks=torch.linspace(-1, 1, 16, device=DEV), num_splits=3, return_lse=True)
    kp, vp, table = _paged(k, v, lens, 2, 128, page, "plhe", 3 * CAP // page + 5, seed=1)
    o, lse = pkg.paged_decode_attention(q, kp, vp, table, seqlens, **kw)
    kp2, vp2, table2 = _paged(k, v, lens, 2, 128, page, "phle", 4 * CAP // page + 11, seed=2)     # the same keys elsewhere in a larger pool
    assert not torch.equal(table, table2)
    o2, lse2 = pkg.paged_decode_attention(q, kp2, vp2, table2, seqlens, **kw)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    for b in range(B):
        ob, lb = pkg.paged_decode_attention(q[b:b + 1], kp, vp, table[b:b + 1], seqlens[b:b + 1], **kw)
        assert torch.equal(ob[0], o[b]) and torch.equal(lb[0], lse[b]), b


def test_a_captured_call_follows_seqlens_the_table_and_the_pages(pkg):
    E, dt, G, QL, page = 64, "bf16", 8, 1, 16
    q, k, v = _inputs(E, dt, G, QL, CAP)
    lens0 = (127, 0, 31)                                 # the first step fills a page of sequences 0 and 2, the second opens their next one
    kp, vp, table = _paged(k, v, lens0, QL, None, page, "plhe", 3 * CAP // page + 5, seed=3)
    free = [p for p in range(kp.size(0)) if p not in set(table.flatten().tolist())]
    lens = torch.tensor(lens0, dtype=torch.int32, device=DEV)
    splits, nbytes = pkg.paged_decode_attention_plan(q, kp, vp, table, num_splits=3)
    assert (splits, nbytes) == (3, 4 * B * KH * G * QL * 3 * (E + 2))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    o, lse = torch.empty_like(q), torch.empty(q.shape[:3], dtype=torch.float32, device=DEV)
    call = lambda o, lse: pkg.paged_decode_attention_into(o, lse, q, kp, vp, table, lens, num_splits=3, workspace=ws)
    call(o, lse)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(o, lse)
    opened = 0
    for step in range(3):                                # a decode step: one more row per sequence, in a new page where the last one is full
        for b, n in enumerate(lens.tolist()):
            if n % page == 0:
                table[b, n // page], opened = free.pop(), opened + 1
            pg = int(table[b, n // page])
            kp[pg, :, n % page], vp[pg, :, n % page] = k[b, :, n], v[b, :, n]
        lens += 1
        a, c = (int(x) for x in table[0, step:step + 2])  # two pages of sequence 0 change places in the pool
        for pool in (kp, vp):
            pool[[a, c]] = pool[[c, a]]
        table[0, step], table[0, step + 1] = c, a
        graph.replay()
        torch.cuda.synchronize()
        o_ref, lse_ref = ref_decode(_f64(q), _f64(_gather(kp, table)), _f64(_gather(vp, table)), lens.tolist(), None, None)
        _judge(f"replay {step}", dt, o, lse, o_ref, lse_ref)
        eager = call(torch.empty_like(o), torch.empty_like(lse))
        assert torch.equal(eager[0], o) and torch.equal(eager[1], lse), step
    assert opened == 3                                   # sequence 1 at its first key, sequences 0 and 2 at a page edge
