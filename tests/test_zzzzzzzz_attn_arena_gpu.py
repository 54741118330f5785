"""The memory contract of flash_attention on the GPU, one case per kernel form: every tensor of a call lives in a guarded arena
(tests/arena.py) and the call is compared BIT FOR BIT with the same call on fresh allocations under the same knobs.

The attention kernels read past their tensors on purpose (LDS-DMA through buffer descriptors whose out-of-range rows read as zeros, a
backward DMA that is not clamped at the end of the stream, one descriptor over the q-heads of a kv head whose ragged tail is masked
only by the padding rows of the workspace) and clamp or zero-fill elsewhere.  On fresh, 512-byte aligned allocations with slack and
finite stale data behind them none of that can be seen going wrong; next to a NaN (0 * NaN) or a zero row constant (P = exp(s)) it
is a wrong gradient.  Per case:

  (a) outputs own exactly their bytes: o, ms, ls / dq, dk, dv, dpair, dsinks embedded with 0xFF and with 0x00 are the fresh bits
      (dead rows included: their NaN and ms = -inf are written, not left over) and no byte outside them changes;
  (b) inputs are read inside their bytes and never written: q, k, v, dO, the forward's o, ms, ls, pair, kpad_mask, sinks embedded
      with 0xFF give the fresh bits, and their arenas are byte for byte what they were;
  (c) the workspace is scratch: exactly bwd_workspace_bytes inside guards, filled with 0xFF, with 0x00, and by the backward of another
      problem (longer QL, one head, another dtype), gives the fresh bits, the guards untouched -- with a pair bias for both sizes;
  (d) ms, ls (element size) and sinks, dsinks (4 bytes) may start at any element.

Then the offset pair bias (pair / dpair need the element size only: a batch slice of a bias starts at any element) and the sharded
call with a pair bias, which hands the library exactly such slices.

The file name sorts behind every other test file for the reason tests/test_residual_addnorm_gpu.py gives.

Measured on an MI355X: the whole file (68 tests) takes 4 s; the slowest test 0.8 s (the first sharded call), the two persistent cases
(16 MiB per tensor) 0.2-0.3 s each.
"""
import functools
from collections import namedtuple
from importlib import import_module

import numpy as np
import pytest
import torch

from arena import FILLS, embed, same_bits, untouched
from attn_ref import inputs

pytestmark = pytest.mark.gpu

DUO, W64, SPLIT, ROW32, GENERIC, CAPPED = ("fa_fwd_duo_kernel", "fa_fwd_w64_kernel", "fa_fwd_split_kernel", "fa_fwd_kernel",
                                           "fa_fwd_generic_kernel", "fa_fwd_cap_kernel")
W64_KV, W64_Q, TILED_KV, TILED_Q = "fa_bwd_w64_kernel<dK/dV>", "fa_bwd_w64_kernel<dQ>", "fa_bwd_dkdv_kernel", "fa_bwd_dq_kernel"

Case = namedtuple("Case", "id form knobs dt E QL KL QH KH B causal want window pad sinks softcap pair staged")


def _c(id, form, knobs, dt, E, QL, KL, QH, KH, B, causal, want, window=None, pad=None, sinks=False, softcap=None, pair=False,
       staged=False):
    return Case(id, form, knobs, dt, E, QL, KL, QH, KH, B, causal, want, window, pad, sinks, softcap, pair, staged)


# The forms of the forward (`form`: the name the host file's table test looks for), pinned through the knobs as FORMS of
# tests/test_sinks_gpu.py pins them; lengths ragged (neither QL nor KL a multiple of 32; KL % 64 == 0 with a ragged QL where the form
# exists in plain mode only); B >= 2 or QH > KH everywhere; GQA, key padding ("lens": a prefix per batch, "left": the first 70 keys
# of the last batch hidden -- dead rows under a causal mask), sinks and causal in turn.
ROW32_KNOBS = dict(fwd_duo=0, fwd_w64=0, fwd_split=0)
FWD_CASES = [
    _c("duo-e128", "duo e128", dict(fwd_duo=1), "bf16", 128, 300, 333, 2, 1, 2, True, DUO),
    _c("duo-e32", "duo e32", dict(fwd_duo=1), "f16", 32, 270, 333, 4, 4, 2, False, DUO, pad="lens"),
    _c("duo-nz2", "duo e64 rows64", dict(fwd_duo=2), "bf16", 64, 300, 320, 4, 2, 2, False, DUO),
    _c("duo-nz1", "duo e64 rows32", dict(fwd_duo=3), "bf16", 64, 301, 333, 4, 2, 1, True, DUO, sinks=True),
    _c("w64-plain", "w64 plain", dict(fwd_duo=0, fwd_w64=1), "bf16", 64, 300, 256, 4, 2, 1, False, W64),
    _c("w64-masked", "w64 masked kpad", dict(fwd_duo=0, fwd_w64=1, fwd_persist=0), "f16", 128, 300, 333, 2, 1, 2, True, W64, pad="left",
       sinks=True),
    _c("w64-e256", "w64 e256", dict(fwd_w64=1), "bf16", 256, 300, 333, 2, 2, 2, False, W64),
    _c("split", "split", dict(fwd_duo=0, fwd_w64=0, fwd_split=1), "bf16", 64, 300, 256, 2, 2, 2, False, SPLIT),
    _c("row32-nw4", "row32 4 waves", dict(fwd_nw=4, **ROW32_KNOBS), "bf16", 64, 300, 333, 4, 2, 1, False, ROW32),
    _c("row32-nw8", "row32 8 waves", dict(fwd_nw=8, **ROW32_KNOBS), "f16", 64, 301, 335, 2, 2, 2, True, ROW32, pad="left"),
    _c("row32-win", "row32 window", dict(), "f16", 64, 300, 333, 4, 2, 1, True, ROW32, window=(127, 0)),
    _c("row32-cap", "row32 softcap", dict(), "bf16", 128, 270, 301, 2, 2, 2, False, CAPPED, softcap=30.0, pad="lens"),
    _c("row32-sinks", "row32 sinks", dict(**ROW32_KNOBS), "bf16", 64, 333, 300, 6, 2, 1, True, ROW32, sinks=True),
    _c("row32-f32", "row32 f32 e128", dict(), "f32", 128, 300, 333, 2, 1, 2, True, ROW32, pad="lens", sinks=True),
    _c("row32-pair", "row32 pair", dict(), "bf16", 64, 205, 147, 4, 2, 2, False, ROW32, pair=True),
    _c("generic", "generic e8", dict(), "bf16", 8, 300, 271, 4, 2, 1, True, GENERIC, sinks=True),
    # the block list needs 256 CUs, B x QH columns in eighths and whole steps of 32 blocks per XCD (persist_list, csrc/fa_launch.hpp):
    # the grid of test_persistent_block_list_is_bitwise_the_one_block_per_workgroup_launch -- 64 columns of 8 blocks, 2 steps
    _c("persist", "persistent", dict(fwd_duo=2, fwd_persist=1), "f16", 64, 2048 - 13, 2048 - 37, 16, 4, 4, True, DUO),
]

# The forms of the backward, as BWD of tests/test_sinks_gpu.py pins them (the hook tells the w64 kernels from the tiled ones, per
# pass; which shape of either runs is the knobs').  bwd_narrow = 0: at these sizes the launcher would take the narrow shape itself.
BWD_CASES = [
    _c("w64-fused", "w64 fused", dict(bwd_w64=1, bwd_narrow=0, bwd_persist=0), "bf16", 64, 301, 333, 4, 2, 2, True, (W64_KV, W64_Q),
       pad="left", sinks=True),
    _c("w64-pre", "w64 preprocess kept", dict(bwd_w64=4, bwd_narrow=0), "f16", 128, 270, 301, 2, 1, 2, False, (W64_KV, W64_Q), pad="lens",
       sinks=True),
    _c("w64-dkdv-only", "w64 dkdv only", dict(bwd_w64=2, bwd_narrow=0), "bf16", 128, 301, 270, 4, 2, 1, True, (W64_KV, TILED_Q)),
    _c("w64-dq-only", "w64 dq only", dict(bwd_w64=3, bwd_narrow=0), "bf16", 64, 333, 301, 2, 2, 2, False, (TILED_KV, W64_Q), pad="lens"),
    _c("w64-narrow", "w64 narrow", dict(bwd_w64=1, bwd_narrow=1), "bf16", 64, 301, 333, 6, 2, 1, True, (W64_KV, W64_Q)),
    _c("w64-persist", "w64 persistent", dict(bwd_w64=1, bwd_narrow=0, bwd_persist=1), "bf16", 64, 2048 - 13, 2048 - 37, 16, 16, 4, True,
       (W64_KV, W64_Q)),
    _c("w64-e256", "w64 e256", dict(bwd_w64=1), "f16", 256, 270, 301, 4, 2, 1, True, (W64_KV, W64_Q)),
    _c("tiled-nw4", "tiled 4 waves", dict(bwd_w64=0, bwd_nw=4), "bf16", 64, 301, 333, 4, 2, 2, True, (TILED_KV, TILED_Q), pad="left"),
    _c("tiled-nw8", "tiled 8 waves", dict(bwd_w64=0, bwd_nw=8), "f16", 32, 301, 333, 4, 2, 1, False, (TILED_KV, TILED_Q)),
    _c("tiled-big7", "tiled e128 big7", dict(bwd_w64=0, bwd_big7=1), "bf16", 128, 301, 333, 4, 2, 2, True, (TILED_KV, TILED_Q),
       pad="lens"),
    _c("tiled-f32-e128", "tiled f32 e128", dict(), "f32", 128, 270, 301, 4, 2, 1, True, (TILED_KV, TILED_Q), sinks=True),
    _c("tiled-f32-e256", "tiled f32 e256", dict(), "f32", 256, 141, 173, 2, 1, 2, False, (TILED_KV, TILED_Q), pad="lens"),
    _c("window", "window body", dict(), "bf16", 64, 301, 333, 4, 2, 1, True, (TILED_KV, TILED_Q), window=(127, 0)),
    _c("cap", "cap body", dict(), "f16", 128, 270, 301, 2, 2, 2, False, (TILED_KV, TILED_Q), softcap=30.0, pad="lens"),
    _c("pair-direct", "pair direct", dict(), "bf16", 64, 205, 147, 4, 2, 2, False, (TILED_KV, TILED_Q), pair=True),
    _c("pair-staged", "pair staged", dict(), "f32", 32, 205, 147, 4, 4, 2, True, (TILED_KV, TILED_Q), pair=True, staged=True, sinks=True),
    _c("generic", "generic e8", dict(), "f16", 8, 300, 271, 4, 2, 1, True, (TILED_KV, TILED_Q), pad="lens"),
]

# check (d): one forward and one backward case per dtype, all with sinks
ELEMENT_ALIGNED_FWD = ("row32-sinks", "w64-masked", "row32-f32")
ELEMENT_ALIGNED_BWD = ("w64-fused", "w64-pre", "tiled-f32-e128")

IN_FWD = ("q", "k", "v", "pair", "mask", "sinks")
IN_BWD = IN_FWD + ("do", "o", "ms", "ls")


def case_desc(pkg, c):
    L = pkg._lib
    return L.FaDesc(dtype={"f32": L.NNOP_F32, "f16": L.NNOP_F16, "bf16": L.NNOP_BF16}[c.dt], emb=c.E, ql=c.QL, kl=c.KL, qh=c.QH, kh=c.KH,
                    batch=c.B, causal=int(c.causal), emb_k=c.E, emb_v=c.E, kl_v=c.KL, kh_v=c.KH)


def fwd_hook(pkg, c):
    return pkg._lib.fwd_form(case_desc(pkg, c), has_pair=c.pair, has_mask=c.pad is not None, window=c.window, softcap=c.softcap)


def bwd_hook(pkg, c):
    return pkg._lib.bwd_kernels(case_desc(pkg, c), has_pair=c.pair, has_mask=c.pad is not None, window=c.window, softcap=c.softcap)


def is_ragged(c):
    """neither length a multiple of 32, or -- for a form taken in plain mode -- whole 64-key tiles with a ragged QL"""
    return c.QL % 32 != 0 and (c.KL % 32 != 0 or c.KL % 64 == 0)


def _problem(c, dev):
    """the case's inputs (generated once per case; the tests only ever copy them)"""
    return dict(_problem_of(c._replace(knobs=None, want=None), dev))


@functools.lru_cache(maxsize=None)
def _problem_of(c, dev):
    d = inputs(("arena", c.id, c.dt, c.E), c.B, c.QH, c.KH, c.QL, c.KL, c.E, c.dt, dev, pair=c.pair, pad=c.pad == "lens",
               sinks="mix" if c.sinks else None)
    if c.pad == "left":
        m = np.ones((c.B, c.KL), dtype=bool)
        m[-1, :70] = False
        d["mask"] = torch.tensor(m).to(dev)
    d.setdefault("sinks", None)
    return d


def _att(pkg):
    return import_module(pkg.__name__ + ".attention")


def _opts(c):
    return dict(causal=c.causal, window=c.window, softcap=c.softcap)


def _fwd(pkg, c, out, T):
    _att(pkg).fa_fwd_into(out["o"], out["ms"], out["ls"], T["q"], T["k"], T["v"], T["pair"], kpad_mask=T["mask"], sinks=T["sinks"],
                          **_opts(c))
    torch.cuda.synchronize()


def _bwd(pkg, c, out, ws, T):
    _att(pkg).fa_bwd_into(out["dq"], out["dk"], out["dv"], out.get("dpair"), ws, T["do"], T["o"], T["ms"], T["ls"], T["q"], T["k"],
                          T["v"], T["pair"], kpad_mask=T["mask"], sinks=T["sinks"], dsinks=out.get("dsinks"), **_opts(c))
    torch.cuda.synchronize()


def _fwd_outs(d):
    q = d["q"]
    return dict(o=torch.empty_like(q), ms=torch.empty(q.shape[:3], dtype=q.dtype, device=q.device),
                ls=torch.empty(q.shape[:3], dtype=q.dtype, device=q.device))


def _bwd_outs(d):
    out = dict(dq=torch.empty_like(d["q"]), dk=torch.empty_like(d["k"]), dv=torch.empty_like(d["v"]))
    if d["pair"] is not None:
        out["dpair"] = torch.empty_like(d["pair"])
    if d["sinks"] is not None:
        out["dsinks"] = torch.empty_like(d["sinks"])
    return out


def _ws_bytes(pkg, c, d, staged):
    return _att(pkg).bwd_workspace_bytes(d["q"], d["k"], d["v"], causal=c.causal, pair=staged)


def _embed_all(tensors, names, fill, copy=True, leads=None):
    """{name: view}, {name: arena} of the tensors that are there"""
    views, arenas = {n: None for n in names}, {}
    for n in names:
        if tensors.get(n) is not None:
            views[n], arenas[n] = embed(tensors[n], fill, (leads or {}).get(n, 0), copy=copy)
    return views, arenas


def _check_outputs(got, arenas, fresh, fill, what):
    for n, t in fresh.items():
        assert same_bits(got[n], t), f"{what}: {n} differs from the fresh-allocation run (fill {fill:#04x})"
        assert untouched(arenas[n], got[n], fill), f"{what}: a byte outside {n} changed (fill {fill:#04x})"


def _check_inputs(arenas, before, what):
    for n, a in arenas.items():
        assert torch.equal(a, before[n]), f"{what}: the arena of the input {n} changed"


def _fresh_fwd(pkg, c, d):
    out = _fwd_outs(d)
    _fwd(pkg, c, out, d)
    return out


def _fresh_bwd(pkg, c, d, ws_bytes=None):
    """the forward's residuals joined to the inputs, and the gradients of a call on fresh allocations with a workspace of `ws_bytes`
    (default: the small size unless the case is the staged one)"""
    T = dict(d, **_fresh_fwd(pkg, c, d))
    out = _bwd_outs(T)
    n = _ws_bytes(pkg, c, d, c.staged) if ws_bytes is None else ws_bytes
    _bwd(pkg, c, out, torch.empty(n, dtype=torch.uint8, device=d["q"].device), T)
    return T, out


# ---- forward: (a), (b) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FWD_CASES, ids=lambda c: c.id)
def test_forward_owns_its_outputs_and_only_reads_its_inputs(pkg, dev, tune, c):
    tune(**c.knobs)
    assert fwd_hook(pkg, c) == c.want and is_ragged(c) and (c.B >= 2 or c.QH > c.KH)
    d = _problem(c, dev)
    fresh = _fresh_fwd(pkg, c, d)
    for fill in FILLS:
        T, TA = _embed_all(d, IN_FWD, 0xFF)
        before = {n: a.clone() for n, a in TA.items()}
        out, OA = _embed_all(fresh, ("o", "ms", "ls"), fill, copy=False)
        _fwd(pkg, c, out, T)
        _check_outputs(out, OA, fresh, fill, c.id)
        _check_inputs(TA, before, c.id)


# ---- backward: (a), (b), and the workspace filled like the outputs -------------------------------------------------------------
def _bwd_in_arenas(pkg, c, T0, fresh, fill, ws_bytes, prepare_ws=None, leads=None):
    T, TA = _embed_all(T0, IN_BWD, 0xFF, leads=leads)
    before = {n: a.clone() for n, a in TA.items()}
    out, OA = _embed_all(fresh, tuple(fresh), fill, copy=False, leads=leads)
    ws, WA = embed(torch.empty(ws_bytes, dtype=torch.uint8, device=T0["q"].device), fill, copy=False, row_bytes=40)
    assert ws.data_ptr() % 16 == 0 and ws.numel() == ws_bytes
    if prepare_ws is not None:
        prepare_ws(ws)
    _bwd(pkg, c, out, ws, T)
    _check_outputs(out, OA, fresh, fill, c.id)
    _check_inputs(TA, before, c.id)
    assert untouched(WA, ws, fill), f"{c.id}: a byte outside the workspace changed (fill {fill:#04x})"


@pytest.mark.parametrize("c", BWD_CASES, ids=lambda c: c.id)
def test_backward_owns_its_outputs_and_only_reads_its_inputs(pkg, dev, tune, c):
    tune(**c.knobs)
    assert bwd_hook(pkg, c) == c.want and is_ragged(c) and (c.B >= 2 or c.QH > c.KH)
    d = _problem(c, dev)
    T0, fresh = _fresh_bwd(pkg, c, d)
    for fill in FILLS:
        _bwd_in_arenas(pkg, c, T0, fresh, fill, _ws_bytes(pkg, c, d, c.staged))


# ---- (c) the workspace is scratch ----------------------------------------------------------------------------------------------
def _other_problem_backward(pkg, c, dev):
    """ws -> None: the backward of ANOTHER problem in that workspace -- longer QL, one head, the other element width, E = 16 (the tiled
    kernels with the preprocess launch) -- so that the rows of the workspace hold the finite row constants of other rows.  Its
    workspace is smaller than the case's (one head of at most QLs + 64 padded rows, 8 bytes each)."""
    dt = "f32" if c.dt != "f32" else "bf16"
    o = _c("other", "", dict(), dt, 16, c.QL + 37, 75, 1, 1, 1, False, None)
    d = _problem(o, dev)
    T, _ = _fresh_bwd(pkg, o, d)
    need = _ws_bytes(pkg, o, d, False)

    def run(ws):
        assert need <= ws.numel()
        _bwd(pkg, o, _bwd_outs(T), ws, T)
    return run


@pytest.mark.parametrize("c", BWD_CASES, ids=lambda c: c.id)
def test_backward_workspace_is_scratch(pkg, dev, tune, c):
    dirty = _other_problem_backward(pkg, c, dev)          # (under the default knobs)
    tune(**c.knobs)
    d = _problem(c, dev)
    sizes = {_ws_bytes(pkg, c, d, False)} | ({_ws_bytes(pkg, c, d, True)} if c.pair else set())
    assert not c.pair or len(sizes) == 2
    for ws_bytes in sorted(sizes):
        # (with a pair bias the larger size takes the staged path, other kernels: each size against the fresh run of its own size)
        T0, fresh = _fresh_bwd(pkg, c, d, ws_bytes)
        for fill in FILLS:
            _bwd_in_arenas(pkg, c, T0, fresh, fill, ws_bytes)
        _bwd_in_arenas(pkg, c, T0, fresh, 0x00, ws_bytes, prepare_ws=dirty)


# ---- (d) element-aligned ms, ls, sinks, dsinks ---------------------------------------------------------------------------------
def _by_id(cases, id):
    return next(c for c in cases if c.id == id)


@pytest.mark.parametrize("id", ELEMENT_ALIGNED_FWD)
def test_forward_takes_element_aligned_rows_and_sinks(pkg, dev, tune, id):
    c = _by_id(FWD_CASES, id)
    tune(**c.knobs)
    d = _problem(c, dev)
    es = d["q"].element_size()
    fresh = _fresh_fwd(pkg, c, d)
    T, TA = _embed_all(d, IN_FWD, 0xFF, leads=dict(sinks=4))
    out, OA = _embed_all(fresh, ("o", "ms", "ls"), 0xFF, copy=False, leads=dict(ms=es, ls=es))
    assert out["ms"].data_ptr() % 16 == es and out["ls"].data_ptr() % 16 == es and T["sinks"].data_ptr() % 16 == 4
    _fwd(pkg, c, out, T)
    _check_outputs(out, OA, fresh, 0xFF, id)


@pytest.mark.parametrize("id", ELEMENT_ALIGNED_BWD)
def test_backward_takes_element_aligned_rows_and_sinks(pkg, dev, tune, id):
    c = _by_id(BWD_CASES, id)
    tune(**c.knobs)
    d = _problem(c, dev)
    es = d["q"].element_size()
    T0, fresh = _fresh_bwd(pkg, c, d)
    assert "dsinks" in fresh
    _bwd_in_arenas(pkg, c, T0, fresh, 0xFF, _ws_bytes(pkg, c, d, c.staged), leads=dict(ms=es, ls=es, sinks=4, dsinks=4))


# ---- the offset pair bias --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,E", [("bf16", 32), ("bf16", 64), ("bf16", 128), ("f32", 32), ("f32", 64), ("f32", 128), ("f16", 64)])
def test_offset_bias_is_the_aligned_bias(pkg, dev, dt, E):
    """pair and dpair at 2, 4 and 8 bytes (fp32: 4 and 8) behind a 16-byte boundary: the forward and the direct backward gather and
    scatter the bias element by element wherever it starts, the staged backward's pack / unpack kernels move whole 16-byte vectors
    from an aligned base (QL x QH = 200 x 4 elements per key row: every row starts on a boundary) and single elements from any other
    (csrc/pair_tile.hpp) -- copies either way, so EVERY output is bitwise the aligned run's; nothing sums in another order."""
    c = _c("offset", "", dict(), dt, E, 200, 150, 4, 2, 2, False, None, pair=True)
    d = dict(_problem(c, dev), sinks=None)
    es = d["q"].element_size()
    fresh_f = _fresh_fwd(pkg, c, d)
    T0 = dict(d, **fresh_f)
    sizes = (_ws_bytes(pkg, c, d, False), _ws_bytes(pkg, c, d, True))
    assert sizes[1] > sizes[0]
    fresh_b = []
    for n in sizes:
        out = _bwd_outs(T0)
        _bwd(pkg, c, out, torch.empty(n, dtype=torch.uint8, device=dev), T0)
        fresh_b.append(out)
    for lead in sorted({es, 4, 8} | ({2} if es == 2 else set())):
        pair, PA = embed(d["pair"], 0xFF, lead)
        assert pair.data_ptr() % 16 == lead
        before = PA.clone()
        out = _fwd_outs(d)
        _fwd(pkg, c, out, dict(d, pair=pair))
        for n in out:
            assert same_bits(out[n], fresh_f[n]), (n, lead)
        for n, fresh in zip(sizes, fresh_b):
            out = _bwd_outs(T0)
            out["dpair"], DA = embed(d["pair"], 0xFF, lead, copy=False)
            _bwd(pkg, c, out, torch.empty(n, dtype=torch.uint8, device=dev), dict(T0, pair=pair))
            for name in out:
                assert same_bits(out[name], fresh[name]), (name, lead, n)
            assert untouched(DA, out["dpair"], 0xFF), (lead, n)
        assert torch.equal(PA, before), lead


# ---- a pair bias through the sharded call -----------------------------------------------------------------------------------------
def _eq(a, b):
    return torch.equal(torch.nan_to_num(a.float()), torch.nan_to_num(b.float()))


SHARD_CASES = [
    # B, QH, KH, QL, KL, E, dt, causal
    (2, 2, 2, 255, 255, 64, "bf16", False),      # rank 1's bias starts 255 * 255 * 2 elements in: 4 bytes behind a 16-byte boundary
    (3, 4, 2, 201, 203, 64, "bf16", True),       # GQA 4 / 2, 6 units: world 2 cuts batch 1 between its kv heads, world 3 gives a batch each
]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", SHARD_CASES, ids=lambda c: f"B{c[0]}H{c[1]}-{c[2]}L{c[3]}x{c[4]}")
def test_sharded_pair_bias_is_bitwise_the_unsharded_launch(pkg, dev, case, world):
    """tests/test_shard_gpu.py with a pair bias: shard_views hands the library the batch slice of the bias as a VIEW, which starts
    b0 * KL * QL * QH elements into the tensor -- any element, not a 16-byte boundary -- and copies only a head-sliced one."""
    B, QH, KH, QL, KL, E, dt, causal = case
    rep = QH // KH
    d = inputs(("shard-pair",) + case, B, QH, KH, QL, KL, E, dt, dev, pair=True)
    es = d["pair"].element_size()
    if case == SHARD_CASES[0]:
        assert (d["pair"].data_ptr() + KL * QL * QH * es) % 16 == 4
    q, k, v, pair = (d[n].clone().requires_grad_(True) for n in ("q", "k", "v", "pair"))
    o_full = pkg.flash_attention(q, k, v, pair, causal=causal)
    o_full.backward(d["do"])
    ref = dict(o=o_full.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dpair=pair.grad)

    # the views: a batch-sliced bias stays a view at its element offset, a head-sliced one is not dense (and is copied by the call)
    for rank in range(world):
        for rect in pkg.shard.rectangles(B, KH, world, rank):
            ps = pkg.shard.shard_views(rect, d["q"], d["k"], d["v"], d["pair"])[3]
            whole = rect.kh0 == 0 and rect.kh1 == KH
            assert ps.is_contiguous() == whole
            if whole:
                assert ps.contiguous().data_ptr() == d["pair"].data_ptr() + rect.b0 * KL * QL * QH * es

    # (1) autograd through the rectangle views, rank by rank
    q2, k2, v2, pair2 = (d[n].clone().requires_grad_(True) for n in ("q", "k", "v", "pair"))
    do_units = d["do"].reshape(B * KH, rep, QL, E)
    for rank in range(world):
        lo, hi = pkg.shard.unit_range(B * KH, world, rank)
        local = pkg.shard.flash_attention_sharded(q2, k2, v2, pair2, causal=causal, world=world, rank=rank)
        assert _eq(local, ref["o"].reshape(B * KH, rep, QL, E)[lo:hi]), f"forward, rank {rank}"
        if hi > lo:
            local.backward(do_units[lo:hi])
    for name, t in (("dq", q2.grad), ("dk", k2.grad), ("dv", v2.grad), ("dpair", pair2.grad)):
        assert _eq(t, ref[name]), f"{name} through autograd over the shard views"

    # (2) the explicit forward + backward driver
    for rank in range(world):
        for rect, o, dq, dk, dv, dp in pkg.shard.flash_attention_sharded_fwd_bwd(d["q"], d["k"], d["v"], d["do"], d["pair"],
                                                                                 causal=causal, world=world, rank=rank):
            b, hs, ks = slice(rect.b0, rect.b1), slice(rect.kh0 * rep, rect.kh1 * rep), slice(rect.kh0, rect.kh1)
            assert _eq(o, ref["o"][b, hs]) and _eq(dq, ref["dq"][b, hs]), (rank, rect)
            assert _eq(dk, ref["dk"][b, ks]) and _eq(dv, ref["dv"][b, ks]), (rank, rect)
            assert _eq(dp, ref["dpair"][b, :, :, hs]), (rank, rect)
