"""GPU tests of the paged KV-cache write (include/nnop_hip_paged_kv_write.h).  The reference is a plain Python scatter on the CPU: the
header's per-token loop -- token i of sequence b goes to row p mod page_size of page table[b][p // page_size], p = seqlens[b] - n_b + i,
unless p < 0 or the id lies outside [0, P) -- with `(x.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn)` for an E4M3 pool, applied
to a copy of pools that were filled with random bytes (NaN codes and 16-bit NaNs among them).  Every comparison is of bits and of the
WHOLE pool, so it covers the rows that are written and the rows that are not.  The batch is the smallest that can go wrong: (new tokens,
prefix) = (1, 15) a decode-like token on a page's last row, (0, 5) an empty sequence, (17, 0) a chunk from a page's start over one
boundary, (33, 31) a chunk from mid-page over several.  K and V are always slices of one tensor, with strides of their own.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import itertools

import numpy as np
import pytest
import torch

from util import TORCH_DT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F8 = torch.float8_e4m3fn
NEWS, PREFIXES = (1, 0, 17, 33), (15, 5, 0, 31)
FORMATS = ("16bit", "e4m3-scaled", "e4m3")
scales_of = lambda KH: torch.tensor([0.0043 * 4.6 ** h for h in range(KH)])     # distinct, in [2^-8, 2^8], no powers of two
i32 = lambda x: torch.tensor(x, dtype=torch.int32)

# every (E, type, format) once, the layout, the page size and KH cycling; then the variants, each on more than one combination
GRID = [(E, dt, fmt, ("phle", "plhe")[(n + n // 2) % 2], (16, 64)[(n + n // 4) % 2], (1, 3, 8)[(n + n // 3) % 3], "base")
        for n, (E, dt, fmt) in enumerate(itertools.product((64, 128), ("f16", "bf16"), FORMATS))]
assert all({(c[2], c[i]) for c in GRID} == set(itertools.product(FORMATS, vals)) for i, vals in ((3, ("phle", "plhe")), (4, (16, 64)), (5, (1, 3, 8))))
GRID += [(128, "bf16", "e4m3-scaled", "plhe", 16, 3, "short"), (64, "f16", "16bit", "phle", 64, 8, "short"),
         (64, "f16", "16bit", "phle", 16, 8, "holes"), (64, "bf16", "e4m3", "plhe", 64, 3, "holes"),
         (128, "f16", "e4m3-scaled", "phle", 16, 8, "fused"), (64, "bf16", "16bit", "plhe", 16, 3, "fused"),
         (128, "bf16", "e4m3-scaled", "plhe", 16, 8, "blocks"), (64, "f16", "16bit", "phle", 64, 1, "blocks"),
         (64, "f16", "e4m3", "plhe", 16, 3, "scattered"), (128, "bf16", "16bit", "phle", 16, 3, "scattered")]


def _bits(x, s=None):                                          # what a pool holds of the rows x [..., KH, E]; s [KH]: the rule's one line
    return x.view(torch.int16) if s is None else (x.float() / s[:, None]).clamp(-448, 448).to(F8).view(torch.uint8)


def ref_write(pools, k, v, table, news, lens, sc):
    """the scatter, in place on the CPU pools [P, KH, page, E] (integers: the bits)"""
    P, page, t = pools[0].size(0), pools[0].size(2), 0
    for b, (n, L) in enumerate(zip(news, lens)):
        for p in range(L - n, L):
            pg = int(table[b, p // page]) if p >= 0 else -1
            if 0 <= pg < P:
                for pool, x in zip(pools, (k, v)):
                    pool[pg, :, p % page] = _bits(x[t], sc)
            t += 1


_kv = lambda src, KH: (src[:, -2 * KH:-KH], src[:, -KH:])       # K and V where they lie in a [T, heads, E] projection: its last 2 KH heads
_logical = lambda store, layout: store if layout == "phle" else store.transpose(1, 2)


def _case(E, dt, fmt, layout, page, KH, news=NEWS, prefixes=PREFIXES, seed=0, spare=3, fused=False):
    """CPU: the projection that holds K and V (magnitudes from below the subnormal codes to beyond 448 scales), the scales, the random
    pools' storage, a table of distinct pages from a seeded permutation, cu_seqlens_q, seqlens and the lengths"""
    g = torch.Generator().manual_seed(1000 * E + 10 * KH + seed)
    T, lens = sum(news), tuple(max(c + n, 0) for c, n in zip(prefixes, news))
    sc = None if fmt == "16bit" else scales_of(KH) if fmt == "e4m3-scaled" else torch.ones(KH)
    src = torch.randn(T, (4 + 2 * KH) if fused else 2 * KH, E, generator=g) * torch.exp2(4 * torch.randn(T, 1, 1, generator=g))
    if fmt == "e4m3-scaled":
        src[:, -2 * KH:] *= torch.cat([sc, sc])[:, None]
    max_pages = -(-max(lens) // page) + 1
    P = len(news) * max_pages + spare
    table = torch.randperm(P, generator=g)[:len(news) * max_pages].to(torch.int32).view(len(news), max_pages)
    shape = (P, KH, page, E) if layout == "phle" else (P, page, KH, E)
    stores = [torch.randint(0, 256, shape + (2 if sc is None else 1,), generator=g, dtype=torch.uint8) for _ in range(2)]
    stores = [(s.view(torch.int16) if sc is None else s).squeeze(-1) for s in stores]
    return src.to(TORCH_DT[dt]), sc, stores, table, i32(np.cumsum((0,) + tuple(news))), i32(lens), lens


def _write(pkg, kd, vd, sc, stores, layout, table, cu, seqlens):
    """the call on device copies of the stores (K's pool as float8_e4m3fn, V's as uint8; all-ones scales as None); what it leaves, on the CPU"""
    dev = [s.to(DEV) for s in stores]
    views = [_logical(d.view(kd.dtype if sc is None else t), layout) for d, t in zip(dev, (F8, torch.uint8))]
    kw = {} if sc is None or bool((sc == 1).all()) else dict(k_scale=sc.to(DEV), v_scale=sc.to(DEV))
    assert pkg.paged_kv_cache_write(kd, vd, *views, table.to(DEV), cu.to(DEV), seqlens.to(DEV), **kw) is None
    return [d.cpu() for d in dev]


@pytest.mark.parametrize("E,dt,fmt,layout,page,KH,variant", GRID, ids=["-".join(map(str, c)) for c in GRID])
def test_the_whole_pools_equal_the_cpu_scatters_bit_for_bit(pkg, E, dt, fmt, layout, page, KH, variant):
    BT = pkg._lib_paged_kv_write.BLOCK_TOKENS
    news, prefixes = {"short": (NEWS, (15, 5, -8, 31)), "blocks": ((2 * BT + 3, 0, 5, BT + 1), PREFIXES)}.get(variant, (NEWS, PREFIXES))
    assert variant != "blocks" or (sum(news) > 2 * BT and sum(news) % BT)
    src, sc, stores, table, cu, seqlens, lens = _case(E, dt, fmt, layout, page, KH, news, prefixes, fused=variant == "fused",
                                                      spare=41 if variant == "scattered" else 3)
    if variant == "holes":                                                      # two live entries: a page of another rank, and one past the pool
        table[2, 0], table[3, 47 // page] = -1, stores[0].size(0)
    want = [s.clone() for s in stores]
    ref_write([_logical(w, layout) for w in want], *_kv(src, KH), table, news, lens, sc)
    assert all((w != s).any() for w, s in zip(want, stores))
    got = _write(pkg, *_kv(src.to(DEV), KH), sc, stores, layout, table, cu, seqlens)
    for name, g, w in zip("kv", got, want):
        assert torch.equal(g, w), f"{name}_pages: {int((g != w).sum())} elements differ, first at {(g != w).nonzero()[:1].tolist()}"


@pytest.mark.parametrize("scale", (None, 0.37, 4.0))
@pytest.mark.parametrize("dt,nans", (("bf16", 254), ("f16", 2046)))
def test_every_input_pattern_converts_as_the_rule_says(pkg, dt, nans, scale):
    """All 65536 patterns as ONE write of 512 rows at E = 128 (V in reverse order); the NaN inputs are exactly `nans`."""
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(TORCH_DT[dt]).view(512, 1, 128)
    sc, order = None if scale is None else torch.tensor([scale]), [3, 1, 7, 0, 2, 6, 5, 4]
    pools = [torch.zeros(8, 1, 64, 128, dtype=torch.uint8, device=DEV) for _ in range(2)]
    pkg.paged_kv_cache_write(x.to(DEV), x.flip(0, 2).contiguous().to(DEV), pools[0].view(F8), pools[1], i32([order]).to(DEV), i32([0, 512]).to(DEV),
                             i32([512]).to(DEV), **({} if sc is None else dict(k_scale=sc.to(DEV), v_scale=sc.to(DEV))))
    got_k, got_v = (p.cpu()[order].reshape(-1) for p in pools)
    want, nan = _bits(x, torch.ones(1) if sc is None else sc).reshape(-1), x.float().isnan().reshape(-1)
    assert int(nan.sum()) == nans and len(set(want[~nan].tolist())) == 254      # every finite code is asked for
    for name, got in (("k", got_k), ("v", got_v.flip(0))):
        bad = (got != want) & ~nan
        assert not bad.any(), f"{name}: {int(bad.sum())} patterns differ, the first {[hex(i) for i in bad.nonzero().flatten()[:4].tolist()]}"
        assert bool((got[nan] & 0x7F == 0x7F).all()), f"{name}: a NaN input without a NaN code"


@pytest.mark.parametrize("fmt", ("16bit", "e4m3-scaled"))
def test_a_sequences_bytes_depend_neither_on_the_batch_nor_on_where_its_pages_lie_nor_on_the_run(pkg, fmt):
    E, dt, layout, page, KH, b = 64, "bf16", "plhe", 16, 3, 3
    src, sc, stores, table, cu, seqlens, lens = _case(E, dt, fmt, layout, page, KH)
    pos = torch.arange(lens[b] - NEWS[b], lens[b])
    rows = lambda got, tab: [_logical(g, layout)[tab[pos // page].long(), :, pos % page] for g in got]   # the sequence's rows, gathered
    kd, vd = _kv(src.to(DEV), KH)
    first = _write(pkg, kd, vd, sc, stores, layout, table, cu, seqlens)
    again = _write(pkg, kd, vd, sc, stores, layout, table, cu, seqlens)
    assert all(torch.equal(a, f) for a, f in zip(again, first))
    _, _, stores2, table2, *_ = _case(E, dt, fmt, layout, page, KH, seed=1, spare=29)                     # other bytes, other ids, a larger pool
    assert stores2[0].size(0) > stores[0].size(0) and not torch.equal(table2[b], table[b])
    t0 = int(cu[b])
    alone = _write(pkg, kd[t0:], vd[t0:], sc, stores2, layout, table2[b:b + 1], cu[b:b + 2] - cu[b], seqlens[b:b + 1])
    for f, a in zip(rows(first, table[b]), rows(alone, table2[b])):
        assert torch.equal(f, a)


def test_a_captured_call_follows_the_rows_cu_seqlens_seqlens_the_table_and_the_scales(pkg):
    E, dt, fmt, layout, page, KH = 128, "f16", "e4m3-scaled", "phle", 16, 3
    src, sc, stores, table, cu, seqlens, lens = _case(E, dt, fmt, layout, page, KH)
    srcd, scd, tabd, cud, lend = (t.to(DEV) for t in (src, sc, table, cu, seqlens))
    dev = [s.to(DEV) for s in stores]
    call = lambda pools: pkg.paged_kv_cache_write(*_kv(srcd, KH), pools[0].view(F8), pools[1], tabd, cud, lend, k_scale=scd, v_scale=scd)
    call(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(dev)
    want = [s.clone() for s in stores]
    for d, w in zip(dev, want):
        d.copy_(w)                                                              # the warm-up's writes are gone
    for step, (news, prefixes) in enumerate(((NEWS, PREFIXES), ((20, 30, 1, 0), (0, 7, 40, 9)), ((0, 0, 51, 0), (3, 3, -4, 3)))):
        lens = tuple(max(c + n, 0) for c, n in zip(prefixes, news))
        src = (src * (1 + step)).roll(step, 0)
        if step:                                                                # every page elsewhere, every scale another value
            sc, table = sc * 1.25, table.flatten()[torch.randperm(table.numel(), generator=torch.Generator().manual_seed(step))].view_as(table)
        for d, s in ((srcd, src), (scd, sc), (tabd, table), (cud, i32(np.cumsum((0,) + news))), (lend, i32(lens))):
            d.copy_(s)
        eager = [d.clone() for d in dev]
        graph.replay()
        call(eager)
        torch.cuda.synchronize()
        ref_write(want, *_kv(src, KH), table, news, lens, sc)
        assert all(torch.equal(d.cpu(), w) and torch.equal(e, d) for d, e, w in zip(dev, eager, want)), step
