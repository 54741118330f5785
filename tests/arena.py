"""Guarded arenas for the attention memory-contract tests (test infrastructure, not a test file).

A tensor handed to the library lives inside one uint8 buffer, between two guard bands, and the whole buffer starts out as one
repeated byte:

    | guard | lead | the tensor's bytes | guard |        every byte = fill, then the tensor's bytes = a copy of the tensor

so a store that over-reaches changes a guard byte (`untouched` sees it), an over-read meets the fill instead of allocator slack, and an
output element that nobody writes keeps the fill -- which differs between two runs with different fills.

The guard is a CONDITION, not a measurement: at least 256 rows of the tensor (the largest workgroup block of any attention kernel
form is 256 rows; 224 and 128 for the others) and at least 64 KiB, rounded up to 16 bytes, so that an over-reach by a whole block
still lands inside the allocation and shows as a changed byte, not as a fault.

The fills: 0xFF is a NaN in fp32, fp16 and bf16 (0xFFFF, 0xFFFFFFFF), "valid key" in a bool mask; 0x00 is +0, "padded key", and a
row constant nl = 0 in the backward's workspace (P = exp(s) instead of 0).
"""
import torch

MIN_GUARD = 64 * 1024
GUARD_ROWS = 256
FILLS = (0xFF, 0x00)


def nbytes(t):
    return t.numel() * t.element_size()


def guard_bytes(t, row_bytes=None):
    """The guard in front of and behind `t`: max(256 rows, 64 KiB), a multiple of 16.  A row is the last axis ([.., L, E]: E
    elements; pair [B, KL, QL, QH]: QH; a vector: one element) unless `row_bytes` says otherwise (the workspace: a uint8 vector whose
    rows are the row constants of a query row)."""
    if row_bytes is None:
        row_bytes = (t.shape[-1] if t.dim() >= 2 else 1) * t.element_size()
    return (max(GUARD_ROWS * row_bytes, MIN_GUARD) + 15) & ~15


def embed(t, fill, lead=0, *, copy=True, row_bytes=None):
    """(view, arena): `arena` is one uint8 buffer of guard + lead + nbytes(t) + guard bytes on t's device, every byte = `fill`, its
    base 16-byte aligned; `view` has t's shape and dtype, is contiguous, starts guard + lead bytes in (so view.data_ptr() % 16 ==
    lead % 16) and holds a copy of t -- or, with copy=False (an output), the fill."""
    g = guard_bytes(t, row_bytes)
    n = nbytes(t)
    assert lead >= 0 and lead % t.element_size() == 0, "lead must keep the element alignment"
    arena = torch.full((g + lead + n + g,), fill, dtype=torch.uint8, device=t.device)
    assert arena.data_ptr() % 16 == 0
    view = arena[g + lead:g + lead + n].view(t.dtype).view(t.shape)
    if copy:
        view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == arena.data_ptr() + g + lead
    return view, arena


def span(arena, view):
    """(first byte, one past the last byte) of `view` inside `arena`"""
    lo = view.data_ptr() - arena.data_ptr()
    hi = lo + nbytes(view)
    assert 0 <= lo and hi <= arena.numel()
    return lo, hi


def untouched(arena, view, fill):
    """True when every byte of `arena` outside `view` still holds `fill`."""
    lo, hi = span(arena, view)
    return bool((arena[:lo] == fill).all()) and bool((arena[hi:] == fill).all())


def same_bits(a, b):
    """bit-for-bit equality of two tensors of one shape and dtype (NaN payloads and the sign of zero included)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
