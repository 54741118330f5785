"""GPU tests of MLA decode attention over a paged latent cache (include/nnop_hip_mla_decode.h).  The reference is a plain fp64 softmax over
the keys each row sees, on the latent rows gathered through the block table.  Shapes: 320 keys of table per sequence in pages of 16, 32
and 64 (a tile of 32 keys spans two pages, is one page, is half a page); lengths at a page and a tile edge and one beside each, 0, 1
(below QL) and the whole table; QH 16 (one wave), 48 (a partial head block) and 128 (two head blocks); 1 / 3 / 7 splits (7 leaves chunks
without a tile).  The two LDS images and the table prefetch reach their steady state only over many tiles of one chunk, so the LONG cases
have 1152 keys = 36 tiles, in pages of 16 and 128.
A sequence's live pages are drawn from a seeded permutation of a pool larger than the tables; every table entry without a visible key
names one poison page, and every pool row that no row of its sequence sees -- the rest of a partly filled page, unowned pages, the
poison page -- holds NaN.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

from test_zzzzzzzzzzzz_decode_attn_gpu import _f64, _ratio
from util import TORCH_DT, assert_close, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP, LONG_CAP, B, W, V = 320, 1152, 3, 576, 512
LENS = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, CAP)
HEADS, QLS, SPLITS, PAGES = (16, 48, 128), (1, 2, 3), (1, 3, 7), (16, 32, 64)
LAYOUTS = ("bhle", "blhe")                               # q contiguous; [B, QL, QH, 576] passed transposed
SCALES = (None, 0.1)
NINF = -np.inf

# every (type, QH, QL) twice, the other axes cycling: 36 cases; then the 2 LONG ones
GRID = [(dt, QH, QL, CAP, (LENS[n % 12], LENS[(5 * n + 3) % 12], LENS[(7 * n + 7) % 12]), SPLITS[(n + n // 9) % 3], PAGES[(n + n // 6) % 3],
         LAYOUTS[(n // 5) % 2], SCALES[(n // 2) % 2])
        for n, (dt, QH, QL, _) in enumerate(itertools.product(("f16", "bf16"), HEADS, QLS, range(2)))]
assert all({c[i] for c in GRID} == set(vals) for i, vals in ((0, ("f16", "bf16")), (1, HEADS), (2, QLS), (5, SPLITS), (6, PAGES), (7, LAYOUTS),
                                                              (8, SCALES)))
assert {n for c in GRID for n in c[4]} == set(LENS)
GRID += [("bf16", 128, 1, LONG_CAP, (LONG_CAP, 577, 289), 1, 16, "bhle", None), ("f16", 48, 2, LONG_CAP, (LONG_CAP, 577, 289), 2, 128, "blhe", 0.1)]

_INPUTS = {}


def _inputs(dt, QH, QL, cap, layout="bhle"):
    """q [B, QH, QL, 576] in either layout and the logical latent rows [B, cap, 576], made once per key and left unchanged"""
    key = (dt, QH, QL, cap, layout)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * QH + 10 * QL + cap)
        mk = lambda *s: torch.tensor(rng.standard_normal(s).astype(np.float32)).to(TORCH_DT[dt]).to(DEV)
        _INPUTS[key] = (mk(B, QH, QL, W) if layout == "bhle" else mk(B, QL, QH, W).transpose(1, 2), mk(B, cap, W))
    return _INPUTS[key]


def _paged(c, lens, page, num_pages, seed):
    """the pool (NaN wherever no row looks) and the table: the pages that hold a visible key of a sequence are the next ones of a seeded
    permutation of the pool, taken sequence by sequence in turn; every other entry names the permutation's last page"""
    max_pages = c.shape[1] // page
    perm = np.random.default_rng(seed).permutation(num_pages)
    assert num_pages > B * max_pages
    pool = torch.full((num_pages, page, W), float("nan"), dtype=c.dtype, device=DEV)
    table, free = np.full((len(lens), max_pages), perm[-1], dtype=np.int32), iter(perm[:-1])
    for n, b in itertools.product(range(max_pages), range(len(lens))):
        r1 = min(lens[b], (n + 1) * page) - n * page
        if r1 > 0:
            pg = table[b, n] = int(next(free))
            pool[pg, :r1] = c[b, n * page:n * page + r1]
    return pool, torch.tensor(table, device=DEV)


def ref_mla(q, rows, lens, scale):
    """fp64: row (b, h, i) stands at p = lens[b] - QL + i and sees keys 0 ... p of rows[b]; a row without a key is 0, lse -inf"""
    Bq, QH, QL, _ = q.shape
    o, lse = np.zeros((Bq, QH, QL, V)), np.full((Bq, QH, QL), NINF)
    for b, i in itertools.product(range(Bq), range(QL)):
        n = int(lens[b]) - QL + i + 1
        if n > 0:
            x = q[b, :, i] @ rows[b, :n].T * scale
            w = np.exp(x - x.max(-1, keepdims=True))
            lse[b, :, i] = x.max(-1) + np.log(w.sum(-1))
            o[b, :, i] = (w / w.sum(-1, keepdims=True)) @ rows[b, :n, :V]
    return o, lse


def _ref(q, pool, table, lens, scale=None):
    rows = _f64(pool[table.long()].reshape(table.size(0), -1, W))     # NaN in every row no query sees: the reference reads it too
    return ref_mla(_f64(q), rows, lens, 192 ** -0.5 if scale is None else scale)


def _judge(name, dt, o, lse, o_ref, lse_ref, **case):
    """o per sequence under the type's gate, lse under the "f32" gate; both ratios go to the error log before anything is asserted"""
    assert np.isfinite(o_ref).all()
    got, dead = _f64(lse), lse_ref == NINF
    record_error("mla_decode", dict(name=name, dt=dt, o_ratio=max(_ratio(_f64(o[b]), o_ref[b], dt) for b in range(o_ref.shape[0])),
                                    lse_ratio=_ratio(got[~dead], lse_ref[~dead], "f32"), **case))
    for b in range(o_ref.shape[0]):
        assert_close(f"{name} o[{b}]", o[b], o_ref[b], dt, floor=not o_ref[b].any())
    assert (got[dead] == NINF).all(), f"{name}: lse of a row without a key"
    if (~dead).any():
        assert_close(f"{name} lse", got[~dead], lse_ref[~dead], "f32")


@pytest.mark.parametrize("dt,QH,QL,cap,lens,splits,page,layout,scale", GRID,
                         ids=[f"{c[0]}-H{c[1]}-QL{c[2]}-L{'_'.join(map(str, c[4]))}-s{c[5]}-p{c[6]}-{c[7]}-x{c[8]}" for c in GRID])
def test_parity_against_fp64_with_nan_in_every_unseen_row(pkg, dt, QH, QL, cap, lens, splits, page, layout, scale):
    q, c = _inputs(dt, QH, QL, cap, layout)
    assert q.is_contiguous() == (layout == "bhle" or QL == 1)
    pool, table = _paged(c, lens, page, B * cap // page + 5, seed=page + QH)
    seqlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o, lse = pkg.mla_decode_attention(q, pool, table, seqlens, softmax_scale=scale, num_splits=splits, return_lse=True)
    assert o.shape == (B, QH, QL, V) and o.dtype == q.dtype
    _judge("parity", dt, o, lse, *_ref(q, pool, table, lens, scale), QH=QH, QL=QL, cap=cap, splits=splits, page=page)


def test_the_bits_depend_neither_on_where_the_pages_lie_nor_on_the_batch(pkg):
    q, c = _inputs("bf16", 48, 2, CAP)
    lens, page, kw = (129, 33, CAP), 16, dict(num_splits=3, return_lse=True)
    seqlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    pool, table = _paged(c, lens, page, 3 * CAP // page + 5, seed=1)
    o, lse = pkg.mla_decode_attention(q, pool, table, seqlens, **kw)
    pool2, table2 = _paged(c, lens, page, 4 * CAP // page + 11, seed=2)           # the same rows elsewhere in a larger pool
    assert not torch.equal(table, table2)
    o2, lse2 = pkg.mla_decode_attention(q, pool2.unsqueeze(2), table2, seqlens, **kw)   # and as [P, page, 1, 576]
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    for b in range(B):
        ob, lb = pkg.mla_decode_attention(q[b:b + 1], pool, table[b:b + 1], seqlens[b:b + 1], **kw)
        assert torch.equal(ob[0], o[b]) and torch.equal(lb[0], lse[b]), b


def test_one_split_against_many_and_a_workspace_of_nan(pkg):
    dt, QH, QL = "f16", 128, 2
    q, c = _inputs(dt, QH, QL, CAP)
    lens = (CAP, 129, 2)
    seqlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    pool, table = _paged(c, lens, 32, 3 * CAP // 32 + 5, seed=4)
    o1, l1 = pkg.mla_decode_attention(q, pool, table, seqlens, num_splits=1, return_lse=True)
    o5, l5 = pkg.mla_decode_attention(q, pool, table, seqlens, num_splits=5, return_lse=True)
    _judge("one split", dt, o1, l1, *_ref(q, pool, table, lens))
    for b in range(B):
        assert_close(f"5 splits against 1, o[{b}]", o5[b], _f64(o1[b]), dt)
    assert_close("5 splits against 1, lse", l5, _f64(l1), "f32")
    splits, nbytes = pkg.mla_decode_attention_plan(q, pool, table, num_splits=5)
    assert (splits, nbytes) == (5, 4 * B * QH * QL * 5 * (V + 2))
    ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
    on, ln = pkg.mla_decode_attention(q, pool, table, seqlens, num_splits=5, return_lse=True, workspace=ws)
    assert torch.equal(on, o5) and torch.equal(ln, l5)


def test_a_captured_call_follows_seqlens_the_table_and_the_pages(pkg):
    dt, QH, QL, page = "bf16", 32, 1, 16
    q, c = _inputs(dt, QH, QL, CAP)
    lens0 = (127, 0, 31)                                 # the first step fills a page of sequences 0 and 2, the second opens their next one
    pool, table = _paged(c, lens0, page, 3 * CAP // page + 5, seed=3)
    free = [p for p in range(pool.size(0)) if p not in set(table.flatten().tolist())]
    lens = torch.tensor(lens0, dtype=torch.int32, device=DEV)
    splits, nbytes = pkg.mla_decode_attention_plan(q, pool, table, num_splits=3)
    assert (splits, nbytes) == (3, 4 * B * QH * QL * 3 * (V + 2))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    o, lse = torch.empty(B, QH, QL, V, dtype=q.dtype, device=DEV), torch.empty(B, QH, QL, dtype=torch.float32, device=DEV)
    call = lambda o, lse: pkg.mla_decode_attention_into(o, lse, q, pool, table, lens, num_splits=3, workspace=ws)
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
            pool[int(table[b, n // page]), n % page] = c[b, n]
        lens += 1
        a, d = (int(x) for x in table[0, step:step + 2])  # two pages of sequence 0 change places in the pool
        pool[[a, d]] = pool[[d, a]]
        table[0, step], table[0, step + 1] = d, a
        graph.replay()
        torch.cuda.synchronize()
        _judge(f"replay {step}", dt, o, lse, *_ref(q, pool, table, lens.tolist()))
        eager = call(torch.empty_like(o), torch.empty_like(lse))
        assert torch.equal(eager[0], o) and torch.equal(eager[1], lse), step
    assert opened == 3                                   # sequence 1 at its first key, sequences 0 and 2 at a page edge
