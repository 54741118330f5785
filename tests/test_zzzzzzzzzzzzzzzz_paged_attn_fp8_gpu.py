"""GPU tests of decode attention over a paged FP8 (E4M3) KV cache (include/nnop_hip_paged_attn_fp8.h).  The reference is the tenth
library's test's plain fp64 softmax over the keys a query sees, on the codes gathered through the block table and DEQUANTISED (code
value x scale) and on the rounded q, so it holds no quantisation error and util.py's gates apply as they stand; every case also asks
for the bits of decode_attention_fp8 on the gathered codes at the same split count.  Shapes: 320 keys of table per sequence in pages of
16, 32 and 64 (a tile of 32 keys spans two pages, is one page, is half a page); lengths at a page and a tile edge, at one round of the
four waves and one beside each, 0, 1 and the whole table; 1 / 3 / 7 splits.  A wave consumes a slot of its ring of four tiles that was
refilled twice -- from table entries fetched a refill earlier -- only from 33 tiles per chunk on, so the LONG cases have 1152 keys = 36
tiles, in pages of 16 and 128.  A sequence's live pages are drawn from a seeded permutation of a pool larger than the tables, so
neighbouring keys lie in distant pages and the sequences interleave; every table entry without a visible key names one poison page, and
every pool row that no query of its sequence sees -- the rest of a partly filled page, pages in front of the window, unowned pages, the
poison page -- holds the NaN code 0x7F in K and V.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

from test_zzzzzzzzzzzz_decode_attn_gpu import _f64, _ratio, ref_decode
from test_zzzzzzzzzzzzz_decode_attn_fp8_gpu import SCALES, _deq
from test_zzzzzzzzzzzzzz_paged_attn_gpu import _gather
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

# every (E, type, (G, QL)) twice, the other axes cycling: 32 cases; then the 4 LONG ones
GRID = [(E, dt, G, QL, CAP, (LENS[n % 12], LENS[(5 * n + 3) % 12], LENS[(7 * n + 7) % 12]), SPLITS[(n + n // 9) % 3], WINDOWS[(n // 3) % 4],
         SINKS[(n // 2) % 2], LAYOUTS[(n // 5) % 2], PAGES[(n + n // 6) % 3], SCALES[(n // 7) % 2])
        for n, (E, dt, (G, QL), _) in enumerate(itertools.product((64, 128), ("f16", "bf16"), ROWS, range(2)))]
assert all({c[i] for c in GRID} == set(vals) for i, vals in ((6, SPLITS), (7, WINDOWS), (8, SINKS), (9, LAYOUTS), (10, PAGES), (11, SCALES)))
assert {n for c in GRID for n in c[5]} == set(LENS) and {(c[0], c[10]) for c in GRID} == set(itertools.product((64, 128), PAGES))
GRID += [(E, ("bf16", "f16")[n % 2], 8, 1 + n % 2, LONG_CAP, (LONG_CAP, 577, 289), splits, window, SINKS[n % 2], LAYOUTS[n % 2], page, SCALES[1])
         for n, (E, page, splits, window) in enumerate([(64, 16, 1, None), (64, 128, 1, 900), (128, 128, 1, None), (128, 16, 2, None)])]

_INPUTS = {}


def _inputs(E, dt, G, QL, cap, scales):
    """q, the logical K and V codes [B, KH, cap, E] (standard normal over the scale, cast to E4M3 on the CPU) as uint8, and the two
    scales; made once per key and left unchanged"""
    key = (E, dt, G, QL, cap, scales)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * E + 10 * G + QL)
        q = torch.tensor(rng.standard_normal((B, KH * G, QL, E)).astype(np.float32)).to(TORCH_DT[dt]).to(DEV)
        sc = [None if scales is None else torch.tensor(s, dtype=torch.float32) for s in (scales or (None, None))]
        codes = [(torch.tensor(rng.standard_normal((B, KH, cap, E)).astype(np.float32)) / (1.0 if s is None else s[None, :, None, None]))
                 .to(torch.float8_e4m3fn).view(torch.uint8).to(DEV) for s in sc]
        _INPUTS[key] = (q, *codes, *(None if s is None else s.to(DEV) for s in sc))
    return _INPUTS[key]


def _paged(k, v, lens, QL, window, page, layout, num_pages, seed):
    """the uint8 pools (0x7F wherever no query looks) and the table: the pages that hold a visible key of a sequence are the next ones of
    a seeded permutation of the pool, taken page index by page index over the sequences; every other entry names its last page"""
    cap, E = k.shape[2], k.shape[3]
    max_pages = cap // page
    perm = np.random.default_rng(seed).permutation(num_pages)
    assert num_pages > B * max_pages
    pools = [torch.full((num_pages, KH, page, E) if layout == "phle" else (num_pages, page, KH, E), 0x7F, dtype=torch.uint8, device=DEV)
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


def _judge(name, dt, o, lse, o_ref, lse_ref, **case):
    """o per sequence under the type's gate, lse under the "f32" gate; both ratios go to the error log before anything is asserted"""
    assert np.isfinite(o_ref).all()
    got, dead = _f64(lse), lse_ref == NINF
    record_error("paged_attn_fp8", dict(name=name, dt=dt, o_ratio=max(_ratio(_f64(o[b]), o_ref[b], dt) for b in range(o_ref.shape[0])),
                                        lse_ratio=_ratio(got[~dead], lse_ref[~dead], "f32"), **case))
    for b in range(o_ref.shape[0]):
        assert_close(f"{name} o[{b}]", o[b], o_ref[b], dt, floor=not o_ref[b].any())
    assert (got[dead] == NINF).all(), f"{name}: lse of a row without a key or a sink"
    if (~dead).any():
        assert_close(f"{name} lse", got[~dead], lse_ref[~dead], "f32")


@pytest.mark.parametrize("E,dt,G,QL,cap,lens,splits,window,sinks,layout,page,scales", GRID,
                         ids=[f"E{c[0]}-{c[1]}-G{c[2]}-QL{c[3]}-L{'_'.join(map(str, c[5]))}-s{c[6]}-w{c[7]}-{'sink' if c[8] else 'nosink'}-{c[9]}-"
                              f"p{c[10]}-{'scaled' if c[11] else 'unscaled'}" for c in GRID])
def test_parity_against_fp64_and_the_dense_fp8_calls_bits_with_the_nan_code_in_every_unseen_row(pkg, E, dt, G, QL, cap, lens, splits, window,
                                                                                                sinks, layout, page, scales):
    q, k, v, ks, vs = _inputs(E, dt, G, QL, cap, scales)
    kp, vp, table = _paged(k, v, lens, QL, window, page, layout, B * cap // page + 5, seed=page + E)
    assert kp.stride() != kp.contiguous().stride() or layout == "phle"
    sk = None if sinks is None else torch.tensor(np.resize(np.array(sinks), KH * G), dtype=torch.float32, device=DEV)
    kw = dict(k_scale=ks, v_scale=vs, window_left=window, sinks=sk, num_splits=splits, return_lse=True)
    seqlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o, lse = pkg.paged_decode_attention_fp8(q, kp.view(torch.float8_e4m3fn), vp, table, seqlens, **kw)      # both accepted dtypes
    kd, vd = _gather(kp, table), _gather(vp, table)      # 0x7F in every row no query sees: the reference and the dense call read it too
    o_ref, lse_ref = ref_decode(_f64(q), _deq(kd, ks), _deq(vd, vs), lens, window, None if sk is None else _f64(sk))
    _judge("parity", dt, o, lse, o_ref, lse_ref, E=E, G=G, QL=QL, cap=cap, splits=splits, page=page)
    od, lsed = pkg.decode_attention_fp8(q, kd, vd, seqlens, **kw)
    assert torch.equal(o, od) and torch.equal(lse, lsed), "not the bits of decode_attention_fp8 on the gathered codes"


@pytest.mark.parametrize("E", (64, 128))
def test_the_bits_depend_neither_on_where_the_pages_lie_nor_on_the_batch(pkg, E):
    q, k, v, ks, vs = _inputs(E, "bf16", 8, 2, CAP, SCALES[1])
    lens, page = (129, 33, CAP), 16
    seqlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kw = dict(k_scale=ks, v_scale=vs, window_left=128, sinks=torch.linspace(-1, 1, 16, device=DEV), num_splits=3, return_lse=True)
    kp, vp, table = _paged(k, v, lens, 2, 128, page, "plhe", 3 * CAP // page + 5, seed=1)
    o, lse = pkg.paged_decode_attention_fp8(q, kp, vp, table, seqlens, **kw)
    kp2, vp2, table2 = _paged(k, v, lens, 2, 128, page, "phle", 4 * CAP // page + 11, seed=2)     # the same keys elsewhere in a larger pool
    assert not torch.equal(table, table2)
    o2, lse2 = pkg.paged_decode_attention_fp8(q, kp2, vp2, table2, seqlens, **kw)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    for b in range(B):
        ob, lb = pkg.paged_decode_attention_fp8(q[b:b + 1], kp, vp, table[b:b + 1], seqlens[b:b + 1], **kw)
        assert torch.equal(ob[0], o[b]) and torch.equal(lb[0], lse[b]), b


def test_a_captured_call_follows_seqlens_the_table_the_pages_and_the_scales(pkg):
    E, dt, G, QL, page = 64, "bf16", 8, 1, 16
    q, k, v, ks0, vs0 = _inputs(E, dt, G, QL, CAP, SCALES[1])
    ks, vs = ks0.clone(), vs0.clone()
    lens0 = (127, 0, 31)                                 # the first step fills a page of sequences 0 and 2, the second opens their next one
    kp, vp, table = _paged(k, v, lens0, QL, None, page, "plhe", 3 * CAP // page + 5, seed=3)
    free = [p for p in range(kp.size(0)) if p not in set(table.flatten().tolist())]
    lens = torch.tensor(lens0, dtype=torch.int32, device=DEV)
    splits, nbytes = pkg.paged_decode_attention_fp8_plan(q, kp, vp, table, num_splits=3)
    assert (splits, nbytes) == (3, 4 * B * KH * G * QL * 3 * (E + 2))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    o, lse = torch.empty_like(q), torch.empty(q.shape[:3], dtype=torch.float32, device=DEV)
    call = lambda o, lse: pkg.paged_decode_attention_fp8_into(o, lse, q, kp, vp, table, lens, k_scale=ks, v_scale=vs, num_splits=3, workspace=ws)
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
        (ks, vs)[step % 2][step % KH] *= 1.25            # and one scale value changes
        graph.replay()
        torch.cuda.synchronize()
        o_ref, lse_ref = ref_decode(_f64(q), _deq(_gather(kp, table), ks), _deq(_gather(vp, table), vs), lens.tolist(), None, None)
        _judge(f"replay {step}", dt, o, lse, o_ref, lse_ref)
        eager = call(torch.empty_like(o), torch.empty_like(lse))
        assert torch.equal(eager[0], o) and torch.equal(eager[1], lse), step
    assert opened == 3                                   # sequence 1 at its first key, sequences 0 and 2 at a page edge
