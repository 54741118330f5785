"""GPU tests of split-KV prefill attention over a paged KV cache (include/nnop_hip_paged_prefill_split.h), with the cases, pools, fp64
reference and gates of tests/test_zzzzzzzzzzzzzzz_paged_prefill_gpu.py.  CAP = 640 keys are at most 20 tiles of a block: forced counts of
2 and 3, of 7 (which divides no tile count met here) and of 64 (more chunks than tiles: chunks without a tile beside chunks of one).  New
tokens at the edges of a row block beside prefixes of 0 and 17 (one tile) and of 130 and 257 (many), windows that move a block's first
tile off 0, NaN in every pool row no query sees and in the whole workspace on entry.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

from test_zzzzzzzzzzzz_decode_attn_gpu import _f64
from test_zzzzzzzzzzzzzzz_paged_prefill_gpu import B, CAP, DEV, LAYOUTS, NEWS, PAGES, ROWS, SINKS, _case, _gather, _inputs, _judge, _paged, ref_prefill

pytestmark = pytest.mark.gpu
SPLITS, PFX, WINDOWS = (2, 3, 7, 64), (0, 17, 130, 257), (None, 40, 128)
NEW_IDX = (0, 1, 2, 4, 5)                                # of NEWS(TB): 0, 1, TB - 1, TB + 1, 2 TB + 3

# every (E, type, G) three times, the other axes cycling: (E, dt, G, splits, news index per sequence, prefix per sequence, window, sinks,
# layout, page); then a sequence with fewer keys than new tokens (its first rows stand below 0)
GRID = [(E, dt, G, SPLITS[(n + n // 4) % 4], tuple(NEW_IDX[(2 * n + 3 * b) % 5] for b in range(B)), tuple(PFX[(n + 3 * b + n // 4) % 4] for b in range(B)),
         WINDOWS[(n + n // 3) % 3], SINKS[(n // 2) % 2], LAYOUTS[(n // 3) % 2], PAGES[(n + n // 6) % 3])
        for n, (E, dt, G, _) in enumerate(itertools.product((64, 128), ("f16", "bf16"), (5, 8), range(3)))]
assert all({c[i] for c in GRID} == set(vals) for i, vals in ((3, SPLITS), (6, WINDOWS), (7, SINKS), (8, LAYOUTS), (9, PAGES)))
assert {i for c in GRID for i in c[4]} == set(NEW_IDX) and {x for c in GRID for x in c[5]} == set(PFX) and any(0 in c[4] for c in GRID)
assert {(c[0], c[3]) for c in GRID} == set(itertools.product((64, 128), SPLITS))
GRID.append((128, "bf16", 8, 7, (4, 1, 5, 2), (-9, 0, -40, 33), 40, SINKS[1], "plhe", 16))
IDS = [f"E{c[0]}-{c[1]}-G{c[2]}-s{c[3]}-n{'_'.join(map(str, c[4]))}-c{'_'.join(map(str, c[5]))}-w{c[6]}-{'sink' if c[7] else 'nosink'}-{c[8]}-p{c[9]}"
       for c in GRID]


def _nan_workspace(pkg, q, kp, vp, table, window, splits):
    got, nbytes = pkg.paged_prefill_attention_split_plan(q, kp, vp, table, window_left=window, num_splits=splits)
    assert (got, nbytes) == (splits, 4 * q.shape[0] * q.shape[1] * splits * (q.shape[2] + 2) if splits > 1 else 0)
    return torch.full((nbytes // 4,), float("nan"), device=DEV)


@pytest.mark.parametrize("E,dt,G,splits,news,prefixes,window,sinks,layout,page", GRID, ids=IDS)
def test_parity_against_fp64_at_forced_split_counts_with_nan_in_the_workspace(pkg, E, dt, G, splits, news, prefixes, window, sinks, layout, page):
    news = tuple(NEWS(ROWS // G)[i] for i in news)
    q, kp, vp, table, cu, seqlens, kw, lens = _case(E, dt, G, news, prefixes, window, sinks, layout, page)
    ws = _nan_workspace(pkg, q, kp, vp, table, window, splits)
    o, lse = pkg.paged_prefill_attention_split(q, kp, vp, table, cu, seqlens, num_splits=splits, workspace=ws, **kw)
    assert o.shape == q.shape and lse.shape == q.shape[:2]
    ref = ref_prefill(_f64(q), _gather(kp, table), _gather(vp, table), news, lens, window, None if sinks is None else _f64(kw["sinks"]))
    assert ref[2].any() == any(c < 0 for c in prefixes)
    _judge("split parity", dt, o, lse, ref, news, E=E, G=G, page=page, splits=splits)


@pytest.mark.parametrize("E,dt,G,splits,news,prefixes,window,sinks,layout,page", GRID[::6], ids=IDS[::6])
def test_one_split_is_the_unsplit_call_bit_for_bit(pkg, E, dt, G, splits, news, prefixes, window, sinks, layout, page):
    news = tuple(NEWS(ROWS // G)[i] for i in news)
    q, kp, vp, table, cu, seqlens, kw, lens = _case(E, dt, G, news, prefixes, window, sinks, layout, page)
    assert pkg.paged_prefill_attention_split_plan(q, kp, vp, table, window_left=window, num_splits=1) == (1, 0)
    o, lse = pkg.paged_prefill_attention_split(q, kp, vp, table, cu, seqlens, num_splits=1, **kw)
    o1, lse1 = pkg.paged_prefill_attention(q, kp, vp, table, cu, seqlens, **kw)
    assert torch.equal(o, o1) and torch.equal(lse, lse1)


def test_the_bits_depend_neither_on_where_the_pages_lie_nor_on_the_workspace_nor_on_the_batch(pkg):
    news, prefixes, splits = (35, 16, 1, 17), (130, 0, 257, 63), 3
    q, kp, vp, table, cu, seqlens, kw, lens = _case(64, "bf16", 8, news, prefixes, 128, SINKS[1], "plhe", 16)
    kw["num_splits"] = splits
    o, lse = pkg.paged_prefill_attention_split(q, kp, vp, table, cu, seqlens, **kw)
    _, kp2, vp2, table2, *_ = _case(64, "bf16", 8, news, prefixes, 128, SINKS[1], "phle", 16, seed=1, spare=47)   # the same keys elsewhere
    assert not torch.equal(table, table2)
    ws = _nan_workspace(pkg, q, kp, vp, table, 128, splits)
    for pools, fill in (((kp2, vp2, table2), 0.0), ((kp, vp, table), float("nan"))):   # a zeroed workspace, then one full of NaN
        o2, lse2 = pkg.paged_prefill_attention_split(q, *pools, cu, seqlens, workspace=ws.fill_(fill), **kw)
        assert torch.equal(o2, o) and torch.equal(lse2, lse)
    for b in range(B):
        s = slice(int(cu[b]), int(cu[b + 1]))
        ob, lb = pkg.paged_prefill_attention_split(q[s], kp, vp, table[b:b + 1], cu[b:b + 2] - cu[b], seqlens[b:b + 1], **kw)
        assert torch.equal(ob, o[s]) and torch.equal(lb, lse[s]), b
    # the automatic count is the plan's: 35 + 16 + 1 + 17 tokens in 2 (4 + 4) workgroups, 20 tiles without a window
    auto = pkg.paged_prefill_attention_split_plan(q, kp, vp, table)[0]
    oa, la = pkg.paged_prefill_attention_split(q, kp, vp, table, cu, seqlens, **dict(kw, window_left=None, num_splits=None))
    of, lf = pkg.paged_prefill_attention_split(q, kp, vp, table, cu, seqlens, **dict(kw, window_left=None, num_splits=auto))
    assert auto == CAP // 32 // pkg._lib_paged_prefill_split.MIN_CHUNK_TILES and torch.equal(oa, of) and torch.equal(la, lf)


def test_a_captured_call_follows_cu_seqlens_seqlens_the_table_and_the_pages(pkg):
    E, dt, G, page, T, splits = 64, "bf16", 8, 16, 70, 3
    q, k, v = _inputs(E, dt, G)
    q = q[:T]
    kp, vp, table = _paged(k, v, (1,) * B, (CAP,) * B, None, page, "plhe", B * CAP // page + 5, seed=3)   # every key of every sequence
    cu, seqlens = (torch.zeros(n, dtype=torch.int32, device=DEV) for n in (B + 1, B))
    ws = _nan_workspace(pkg, q, kp, vp, table, 100, splits)
    o, lse = torch.empty_like(q), torch.empty(q.shape[:2], dtype=torch.float32, device=DEV)
    call = lambda o, lse: pkg.paged_prefill_attention_split_into(o, lse, q, kp, vp, table, cu, seqlens, window_left=100, num_splits=splits, workspace=ws)
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
        _judge(f"split replay {step}", dt, o, lse, ref_prefill(_f64(q), _gather(kp, table), _gather(vp, table), news, lens, 100, None), news)
        eager = call(torch.empty_like(o), torch.empty_like(lse))
        assert torch.equal(eager[0], o) and torch.equal(eager[1], lse), step
