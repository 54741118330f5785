"""Sliding-window (local) attention on the GPU: parity with the fp64 oracle under a 0 / -inf window bias (tests/attn_ref.py),
exact and normalised windows, repeatability, autograd and sharding.  Window semantics: include/nnop_hip.h (nnop_fa_opts)."""
import pytest
import torch

from attn_ref import check_parity, inputs

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
EMBS = [16, 32, 64, 128, 256, 8]                 # 8: the plain-HIP kernels
LENS = [(63, 65), (517, 517), (65, 63), (1100, 517), (517, 1100), (1, 63)]


def _windows(QL):
    return [(0, 0), (1, 0), (63, -1), (64, 0), (100, 37), (-1, 17), (QL - 2, -1)]


def _normalises_away(QL, KL, causal, w):
    """the library's rule (FaWindow, csrc/fa_launch.hpp): does the window remove no key of this problem?"""
    left_off = w[0] < 0 or w[0] >= QL - 1
    right_off = w[1] < 0 or w[1] >= KL - 1 or (causal and w[1] >= 0)
    return left_off and right_off


def _grid():
    """the product dtype x E x causal x window x lengths, pruned the way test_reference_grids_gpu.py prunes: every E meets every
    dtype, both causal settings and, over the E axis, every window and length pair.  Every case stays windowed after
    normalisation (the next window / length of the cycle is taken where one would not)."""
    out = []
    i = 0
    for E in EMBS:
        for dt in DTYPES:
            for causal in (False, True):
                for j in range(len(LENS) * 7):
                    QL, KL = LENS[(i + EMBS.index(E) + j // 7) % len(LENS)]
                    if E >= 128 and QL * KL > 600 * 600:
                        QL, KL = (QL // 2 + 1, KL // 2 + 1)      # the fp64 oracle is the time here, not the kernel
                    w = _windows(QL)[(i + j) % 7]
                    if not _normalises_away(QL, KL, causal, w):
                        break
                out.append((dt, E, causal, QL, KL, w))
                i += 1
    return out


def _wide_grid():
    """windows wide enough that waves of the pipelined 16-bit kernels (E <= 64) have a PLAIN run of fully visible tiles after a
    general run (the left window edge) and before another (the right edge / diagonal): 32-row waves, 64-key tiles, a window of
    >= 255 keys leaves >= 3 full tiles per wave.  Key padding keeps the general interval's validity words in play."""
    out = []
    wins = [(300, 0), (255, 37), (600, -1)]
    i = 0
    for dt in ("bf16", "f16"):
        for E in (16, 32, 64):
            for causal in (False, True):
                QL, KL = (1100, 1100) if i % 2 == 0 else (1100, 1000)
                out.append((dt, E, causal, QL, KL, wins[i % 3]))
                i += 1
    return out


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "{}-E{}-c{}-L{}x{}-w{}_{}".format(*c[:5], *c[5]))
def test_window_parity(pkg, dev, case):
    dt, E, causal, QL, KL, window = case
    d = inputs(case, 1, 2, 1, QL, KL, E, dt, dev)
    check_parity(pkg, d, dt, causal, window=window)


def test_grids_stay_windowed():
    for dt, E, causal, QL, KL, w in _grid() + _wide_grid():
        assert not _normalises_away(QL, KL, causal, w), (dt, E, causal, QL, KL, w)


@pytest.mark.parametrize("case", _wide_grid(), ids=lambda c: "{}-E{}-c{}-L{}x{}-w{}_{}".format(*c[:5], *c[5]))
def test_window_parity_wide(pkg, dev, case):
    dt, E, causal, QL, KL, window = case
    d = inputs(("wide",) + case, 1, 2, 1, QL, KL, E, dt, dev, pad=True)
    check_parity(pkg, d, dt, causal, window=window)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("E,QL,KL,causal,window,pair,pad", [
    (64, 517, 517, True, (100, 0), False, False),       # GQA 8 / 2
    (32, 300, 517, False, (63, 37), False, True),       # key padding
    (64, 200, 260, False, (40, 17), True, False),       # pair bias (direct path), dpair zero outside the window
    (128, 160, 130, True, (64, -1), True, False),       # pair bias, E = 128 (32-key tiles)
])
def test_window_parity_gqa_padding_pair(pkg, dev, dt, E, QL, KL, causal, window, pair, pad):
    QH, KH = (8, 2) if not pair else (2, 2)
    d = inputs((dt, E, QL, KL, window), 2, QH, KH, QL, KL, E, dt, dev, pair=pair, pad=pad)
    check_parity(pkg, d, dt, causal, window=window)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("E", EMBS)
def test_window_zero_is_exact(pkg, dev, dt, E):
    """window (0, 0): query i sees key i alone -> o = v[i] bitwise, ls = 1 (logits kept tiny so that exp(s - max) is 1 exactly)"""
    B, QH, KH, QL, KL = 2, 4, 2, 200, 260
    d = inputs(("exact", dt, E), B, QH, KH, QL, KL, E, dt, dev)
    q = d["q"] * 2.0 ** -12
    o, ms, ls = pkg._flash_attention(q, d["k"], d["v"], causal=False, window=(0, 0))
    torch.cuda.synchronize()
    vg = d["v"].repeat_interleave(QH // KH, dim=1)[:, :, :QL]
    assert torch.equal(o, vg)
    assert (ls == 1).all()


# shapes that run the duo / w64 / split forms without a window (C2-like, a causal E = 128, a 16-bit E = 32 grid) and the others
NORM_SHAPES = [
    ("bf16", 64, 2048, 2048, 4, 4, 4, False),
    ("bf16", 128, 1024, 1024, 8, 8, 2, True),
    ("f16", 32, 1024, 1024, 8, 8, 8, True),
    ("bf16", 64, 1024, 1024, 8, 2, 2, False),
    ("f32", 64, 600, 700, 2, 2, 2, True),
    ("bf16", 8, 300, 300, 2, 2, 1, False),
    ("bf16", 32, 256, 320, 2, 2, 2, False, True),         # pair bias: the staged backward of the call without a window
    ("f16", 64, 300, 300, 4, 4, 1, True, True),
]


@pytest.mark.parametrize("shape", NORM_SHAPES, ids=lambda s: "{}-E{}-L{}x{}-H{}x{}-B{}-c{}".format(*s) + ("-pair" if len(s) > 8 else ""))
def test_windows_that_normalise_away_are_bitwise_the_unwindowed_call(pkg, dev, shape):
    dt, E, QL, KL, QH, KH, B, causal = shape[:8]
    pair = len(shape) > 8
    d = inputs(shape, B, QH, KH, QL, KL, E, dt, dev, pair=pair)
    q, k, v, do, p = d["q"], d["k"], d["v"], d["do"], d["pair"]
    ref_f = pkg._flash_attention(q, k, v, p, causal=causal)
    ref_b = pkg.grad_flash_attention(do, *ref_f, q, k, v, p, causal=causal)
    windows = [(-1, -1), (QL - 1, -1), (-1, KL - 1), (QL + 3, KL + 9)] + ([(-1, 0), (QL - 1, 5)] if causal else [])
    for w in windows:
        got_f = pkg._flash_attention(q, k, v, p, causal=causal, window=w)
        got_b = pkg.grad_flash_attention(do, *got_f, q, k, v, p, causal=causal, window=w)
        if not pair:
            got_b, ref_b = got_b[:3], tuple(ref_b)[:3]
        for name, a, b in zip(("o", "ms", "ls", "dq", "dk", "dv", "dpair"), tuple(got_f) + tuple(got_b), tuple(ref_f) + tuple(ref_b)):
            assert torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(), b.nan_to_num()), (w, name)


@pytest.mark.parametrize("dt,E,causal,window,pad", [
    ("bf16", 64, True, (127, 0), False),
    ("f32", 128, False, (33, 70), True),
    ("f16", 16, False, (-1, 5), False),
])
def test_windowed_runs_are_repeatable(pkg, dev, dt, E, causal, window, pad):
    d = inputs(("rep", dt, E), 2, 4, 2, 700, 650, E, dt, dev, pad=pad)
    runs = []
    for _ in range(2):
        o, ms, ls = pkg._flash_attention(d["q"], d["k"], d["v"], causal=causal, kpad_mask=d["mask"], window=window)
        g = pkg.grad_flash_attention(d["do"], o, ms, ls, d["q"], d["k"], d["v"], causal=causal, kpad_mask=d["mask"], window=window)
        runs.append([o, ms, ls] + list(g[:3]))
    for a, b in zip(*runs):
        assert torch.equal(a.nan_to_num(), b.nan_to_num())


def test_autograd_matches_grad_flash_attention(pkg, dev):
    d = inputs("autograd", 2, 4, 2, 333, 333, 64, "bf16", dev, pair=True)
    window = (50, 10)
    leaves = [d[n].clone().requires_grad_(True) for n in ("q", "k", "v", "pair")]
    o = pkg.flash_attention(*leaves, causal=True, window=window)
    o.backward(d["do"])
    o2, ms, ls = pkg._flash_attention(d["q"], d["k"], d["v"], d["pair"], causal=True, window=window)
    ref = pkg.grad_flash_attention(d["do"], o2, ms, ls, d["q"], d["k"], d["v"], d["pair"], causal=True, window=window)
    assert torch.equal(o.detach(), o2)
    for leaf, r in zip(leaves, ref):
        assert torch.equal(leaf.grad, r)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_window_is_bitwise_the_unsharded_call(pkg, dev, world):
    from importlib import import_module
    shard = import_module(pkg.__name__ + ".shard")
    d = inputs(("shard", world), 3, 4, 2, 400, 400, 64, "bf16", dev)
    q, k, v, do = d["q"], d["k"], d["v"], d["do"]
    window = (90, 0)
    o, ms, ls = pkg._flash_attention(q, k, v, causal=True, window=window)
    dq, dk, dv, _ = pkg.grad_flash_attention(do, o, ms, ls, q, k, v, causal=True, window=window)
    rep = q.shape[1] // k.shape[1]
    seen = 0
    for rank in range(world):
        for rect, o_r, dq_r, dk_r, dv_r, _ in shard.flash_attention_sharded_fwd_bwd(q, k, v, do, causal=True, world=world,
                                                                                    rank=rank, window=window):
            qs = (slice(rect.b0, rect.b1), slice(rect.kh0 * rep, rect.kh1 * rep))
            ks = (slice(rect.b0, rect.b1), slice(rect.kh0, rect.kh1))
            assert torch.equal(o_r, o[qs]) and torch.equal(dq_r, dq[qs])
            assert torch.equal(dk_r, dk[ks]) and torch.equal(dv_r, dv[ks])
            seen += rect.units
        local = shard.flash_attention_sharded(q, k, v, causal=True, world=world, rank=rank, window=window)
        rects = shard.rectangles(3, 2, world, rank)
        want = [o[r.b0:r.b1, r.kh0 * rep:r.kh1 * rep].reshape(r.units, rep, *o.shape[2:]) for r in rects]
        assert torch.equal(local, torch.cat(want, dim=0))
    assert seen == 3 * 2
