"""CPU tests behind tests/test_zzzzzzzz_attn_arena_gpu.py: the arena harness (tests/arena.py) sees what it claims to see, and the case
tables of the GPU file are what they claim -- every attention kernel form occurs, every case reaches the form it names through the
launcher's own rule (the host-side hooks, no device needed), and every case is ragged and has a next head.

No entry point is called here with made-up addresses: that an offset bias is accepted is tested on the GPU, with real memory."""
import pytest
import torch

import arena
from arena import FILLS, embed, guard_bytes, same_bits, span, untouched
from test_zzzzzzzz_attn_arena_gpu import (BWD_CASES, ELEMENT_ALIGNED_BWD, ELEMENT_ALIGNED_FWD, FWD_CASES, bwd_hook, fwd_hook, is_ragged)

DTYPES = (torch.float32, torch.float16, torch.bfloat16)


# ---- the harness ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_fill_ff_is_nan_and_fill_00_is_zero(dtype):
    v, _ = embed(torch.zeros(3, 5, dtype=dtype), 0xFF, copy=False)
    assert torch.isnan(v).all()
    v, _ = embed(torch.ones(3, 5, dtype=dtype), 0x00, copy=False)
    assert (v == 0).all() and not torch.signbit(v).any()
    m, _ = embed(torch.zeros(2, 7, dtype=torch.bool), 0xFF, copy=False)
    assert m.all()
    m, _ = embed(torch.ones(2, 7, dtype=torch.bool), 0x00, copy=False)
    assert not m.any()


@pytest.mark.parametrize("fill", FILLS)
def test_embed_lays_the_tensor_between_two_guards(fill):
    t = torch.randn(2, 3, 37, 64).to(torch.bfloat16)
    v, a = embed(t, fill)
    g = guard_bytes(t)
    assert g == 64 * 1024 and g % 16 == 0                                   # 256 rows of 128 bytes are less than the floor
    assert a.dtype == torch.uint8 and a.numel() == 2 * g + arena.nbytes(t) and a.data_ptr() % 16 == 0
    assert v.shape == t.shape and v.dtype == t.dtype and v.is_contiguous() and same_bits(v, t)
    assert span(a, v) == (g, g + arena.nbytes(t)) and untouched(a, v, fill)
    # 256 rows, where that is more: fp32 E = 256 rows of 1 KiB; a pair bias row is QH elements, a vector's one element
    assert guard_bytes(torch.empty(2, 2, 9, 256)) == 256 * 1024
    assert guard_bytes(torch.empty(2, 9, 9, 4, dtype=torch.float16)) == 64 * 1024 == guard_bytes(torch.empty(7))
    assert guard_bytes(torch.empty(100, dtype=torch.uint8), row_bytes=1000) == 256 * 1000


@pytest.mark.parametrize("fill", FILLS)
def test_a_planted_byte_anywhere_outside_the_view_is_reported(fill):
    t = torch.randn(4, 33)
    for lead in (0, 4):
        v, a = embed(t, fill, lead)
        lo, hi = span(a, v)
        for at in (lo - 1, hi, 0, a.numel() - 1):        # just in front, just behind, the far end of each guard
            keep = int(a[at])
            a[at] = keep ^ 0x5A
            assert not untouched(a, v, fill), at
            a[at] = keep
            assert untouched(a, v, fill)
        v.fill_(7.0)                                     # writes inside the view are the owner's
        assert untouched(a, v, fill)


def test_an_unwritten_output_element_differs_between_the_two_fills():
    want = torch.randn(5, 16).to(torch.float16)
    runs = []
    for fill in FILLS:
        v, a = embed(want, fill, copy=False)
        v.view(-1)[:-1] = want.view(-1)[:-1]             # a "kernel" that leaves the last element alone
        assert untouched(a, v, fill)
        runs.append(v.clone())
    assert not same_bits(runs[0], runs[1]) and not same_bits(runs[0], want) and not same_bits(runs[1], want)
    assert same_bits(runs[0].view(-1)[:-1], want.view(-1)[:-1])


def test_same_bits_is_bitwise():
    z = torch.zeros(4)
    assert z.equal(-z) and not same_bits(z, -z)
    n = torch.full((4,), float("nan"))
    assert not n.equal(n) and same_bits(n, n.clone())
    assert not same_bits(z, z.to(torch.float16)) and not same_bits(z, torch.zeros(2, 2))


@pytest.mark.parametrize("dtype,leads", [(torch.float32, (0, 4, 8)), (torch.float16, (0, 2, 4, 8)), (torch.bfloat16, (0, 2, 6, 14))],
                         ids=["f32", "f16", "bf16"])
def test_lead_gives_the_stated_address_residue(dtype, leads):
    t = torch.randn(3, 11).to(dtype)
    for lead in leads:
        v, a = embed(t, 0xFF, lead)
        assert v.data_ptr() % 16 == lead % 16 and same_bits(v, t) and untouched(a, v, 0xFF)
    with pytest.raises(AssertionError):
        embed(t, 0xFF, 1)                                # not a whole element


# ---- the case tables -----------------------------------------------------------------------------------------------------------
def _steps(cols, n_blk):
    """persist_list (csrc/fa_launch.hpp) on a 256-CU device with the knob at 1: steps of the block list, 0 = one block per workgroup"""
    per_xcd = (cols // 8) * n_blk
    ok = cols % 8 == 0 and n_blk & (n_blk - 1) == 0 and per_xcd % 32 == 0 and per_xcd // 32 >= 2
    return per_xcd // 32 if ok else 0


b16 = lambda c: c.dt in ("bf16", "f16")
plain = lambda c: not (c.causal or c.pad or c.window or c.softcap or c.pair) and c.KL % 64 == 0
# form -> what the case's knobs and problem must be for the name to be true, beyond the kernel the hook reports (which cannot tell
# the shapes of a form apart: rows per wave, waves per workgroup, the block list)
FWD_FORMS = {
    "duo e128": lambda c: c.knobs.get("fwd_duo") == 1 and c.E == 128 and b16(c),
    "duo e32": lambda c: c.knobs.get("fwd_duo") == 1 and c.E == 32 and b16(c),
    "duo e64 rows64": lambda c: c.knobs.get("fwd_duo") == 2 and c.E == 64 and b16(c),
    "duo e64 rows32": lambda c: c.knobs.get("fwd_duo") == 3 and c.E == 64 and b16(c),
    "w64 plain": lambda c: c.knobs.get("fwd_w64") == 1 and c.E in (64, 128) and plain(c),
    "w64 masked kpad": lambda c: c.knobs.get("fwd_w64") == 1 and c.E in (64, 128) and c.pad is not None,
    "w64 e256": lambda c: c.E == 256 and b16(c),
    "split": lambda c: c.knobs.get("fwd_split") == 1 and c.E <= 64 and plain(c),
    "row32 4 waves": lambda c: c.knobs.get("fwd_nw") == 4 and not (c.window or c.softcap),
    "row32 8 waves": lambda c: c.knobs.get("fwd_nw") == 8 and c.E < 256 and not (c.window or c.softcap),
    "row32 window": lambda c: c.window is not None and c.window[0] < c.QL - 1,
    "row32 softcap": lambda c: bool(c.softcap),
    "row32 sinks": lambda c: c.sinks,
    "row32 f32 e128": lambda c: c.dt == "f32" and c.E == 128,
    "row32 pair": lambda c: c.pair,
    "generic e8": lambda c: c.E == 8,
    "persistent": lambda c: (c.knobs.get("fwd_persist") == 1 and c.knobs.get("fwd_duo") == 2 and c.causal and not c.pad
                             and _steps(c.B * c.QH, (c.QL + 255) // 256) >= 2),
}
w64_b = lambda c: b16(c) and c.E in (64, 128) and not (c.pair or c.window or c.softcap)
wide = lambda c: c.knobs.get("bwd_narrow") == 0 and c.knobs.get("bwd_persist", 0) == 0
BWD_FORMS = {
    "w64 fused": lambda c: c.knobs.get("bwd_w64") == 1 and w64_b(c) and wide(c),
    "w64 preprocess kept": lambda c: c.knobs.get("bwd_w64") == 4 and w64_b(c) and wide(c),
    "w64 dkdv only": lambda c: c.knobs.get("bwd_w64") == 2 and w64_b(c) and wide(c),
    "w64 dq only": lambda c: c.knobs.get("bwd_w64") == 3 and w64_b(c) and wide(c),
    "w64 narrow": lambda c: c.knobs.get("bwd_w64") == 1 and c.knobs.get("bwd_narrow") == 1 and w64_b(c),
    # (the block list runs in the masked kernels only: causal here, without key padding; both passes: columns B x QH and B x KH)
    "w64 persistent": lambda c: (c.knobs.get("bwd_w64") == 1 and c.knobs.get("bwd_persist") == 1 and c.knobs.get("bwd_narrow") == 0
                                 and w64_b(c) and c.causal and not c.pad and _steps(c.B * c.QH, (c.QL + 255) // 256) >= 2
                                 and _steps(c.B * c.KH, (c.KL + 255) // 256) >= 2),
    "w64 e256": lambda c: b16(c) and c.E == 256 and not (c.pair or c.window or c.softcap),
    "tiled 4 waves": lambda c: c.knobs.get("bwd_w64") == 0 and c.knobs.get("bwd_nw") == 4 and b16(c) and c.E <= 64,
    "tiled 8 waves": lambda c: c.knobs.get("bwd_w64") == 0 and c.knobs.get("bwd_nw") == 8 and b16(c) and c.E <= 64 and not c.pair,
    "tiled e128 big7": lambda c: c.knobs.get("bwd_w64") == 0 and c.knobs.get("bwd_big7") == 1 and b16(c) and c.E == 128,
    "tiled f32 e128": lambda c: c.dt == "f32" and c.E == 128,
    "tiled f32 e256": lambda c: c.dt == "f32" and c.E == 256 and not c.pair and not c.softcap,
    "window body": lambda c: c.window is not None and c.window[0] < c.QL - 1 and not c.softcap,
    "cap body": lambda c: bool(c.softcap),
    "pair direct": lambda c: c.pair and not c.staged,
    "pair staged": lambda c: c.pair and c.staged and not (c.window or c.softcap) and c.E in (16, 32, 64, 128),
    "generic e8": lambda c: c.E == 8,
}


@pytest.mark.parametrize("cases,forms", [(FWD_CASES, FWD_FORMS), (BWD_CASES, BWD_FORMS)], ids=["forward", "backward"])
def test_every_form_occurs_once(cases, forms):
    assert sorted(c.form for c in cases) == sorted(forms)
    assert len({c.id for c in cases}) == len(cases)


@pytest.mark.parametrize("c", FWD_CASES, ids=lambda c: c.id)
def test_forward_case_is_what_it_claims(pkg, tune, c):
    tune(**c.knobs)
    assert fwd_hook(pkg, c) == c.want
    assert FWD_FORMS[c.form](c), c.form
    assert is_ragged(c) and (c.B >= 2 or c.QH > c.KH) and c.QH % c.KH == 0


@pytest.mark.parametrize("c", BWD_CASES, ids=lambda c: c.id)
def test_backward_case_is_what_it_claims(pkg, tune, c):
    tune(**c.knobs)
    assert bwd_hook(pkg, c) == c.want
    assert BWD_FORMS[c.form](c), c.form
    assert is_ragged(c) and (c.B >= 2 or c.QH > c.KH) and c.QH % c.KH == 0
    if c.pair:      # the staged path exists for this problem, and only there does the larger workspace differ
        import ctypes as C
        from test_zzzzzzzz_attn_arena_gpu import case_desc
        lib, d = pkg._lib.load(), case_desc(pkg, c)
        assert lib.nnop_fa_bwd_workspace_bytes_pair(C.byref(d)) > lib.nnop_fa_bwd_workspace_bytes(C.byref(d)) > 0


def test_ragged_means_no_whole_tiles():
    from test_zzzzzzzz_attn_arena_gpu import _c
    mk = lambda QL, KL: _c("x", "", {}, "bf16", 64, QL, KL, 2, 2, 2, False, None)
    assert is_ragged(mk(301, 333)) and is_ragged(mk(300, 256))
    assert not is_ragged(mk(320, 333)) and not is_ragged(mk(301, 96)) and not is_ragged(mk(256, 256))


def test_element_aligned_cases_cover_every_dtype_with_sinks():
    for ids, cases in ((ELEMENT_ALIGNED_FWD, FWD_CASES), (ELEMENT_ALIGNED_BWD, BWD_CASES)):
        picked = [c for c in cases if c.id in ids]
        assert len(picked) == len(ids) and sorted(c.dt for c in picked) == ["bf16", "f16", "f32"] and all(c.sinks for c in picked)
