"""Reference of the MXFP4 format of include/nnop_hip_moe_mx.h (test infrastructure, not a test file): the header's definition in numpy.

A block is 32 values along the last axis: 16 bytes of codes (byte j: element 2j in the low nibble, 2j + 1 in the high one) and a scale
byte e.  A code c is E2M1 -- bit 3 the sign, c & 7 the magnitudes of MAGNITUDES -- and e means 2^(e - 127), 255 NaN.

dequant evaluates magnitude 2^(e - 127) in fp64, where it is exact for every (c, e), and rounds once to the target type with torch's
conversion (nearest even, overflow to Inf, subnormals kept); fp64 -> fp32 -> 16 bits rounds once, because whatever fp32 holds exactly of
a two-bit significand it holds without rounding.  quant is the floor rule of OCP MX v1.0 as the header words it, on fp64 copies of the
inputs: scale 2^(floor(log2(amax)) - 2), the nearest magnitude, ties to the even code, saturation at 6, the sign kept."""
import numpy as np

from moe_gemm_ref import round_to

MAGNITUDES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
VALUES = np.concatenate([MAGNITUDES, -MAGNITUDES])                        # the 16 codes; VALUES[8] is -0.0
MIDPOINTS = (MAGNITUDES[1:] + MAGNITUDES[:-1]) / 2                       # 0.25 0.75 1.25 1.75 2.5 3.5 5
BLOCK = 32


def unpack(blocks):
    """uint8 [..., nb, 16] -> codes [..., nb, 32]"""
    b = np.asarray(blocks, np.uint8)
    assert b.shape[-1] == BLOCK // 2
    codes = np.empty(b.shape[:-1] + (BLOCK,), np.uint8)
    codes[..., 0::2], codes[..., 1::2] = b & 15, b >> 4
    return codes


def pack(codes):
    """codes [..., nb, 32] -> uint8 [..., nb, 16]"""
    c = np.asarray(codes, np.uint8)
    return (c[..., 0::2] | (c[..., 1::2] << 4)).astype(np.uint8)


def dequant64(blocks, scales):
    """blocks [..., nb, 16] or [..., nb * 16] beside scales [..., nb] -> fp64 [..., K], exact; NaN for the blocks of scale byte 255"""
    e = np.asarray(scales, np.uint8).astype(np.int64)
    codes = unpack(np.asarray(blocks, np.uint8).reshape(e.shape + (BLOCK // 2,)))
    with np.errstate(invalid="ignore"):
        v = VALUES[codes] * np.where(e == 255, np.nan, np.ldexp(1.0, e - 127))[..., None]
    return v.reshape(v.shape[:-2] + (-1,))


def dequant(blocks, scales, dt):
    """-> the values of type dt as fp64 [..., K]"""
    with np.errstate(over="ignore"):
        return round_to(dequant64(blocks, scales).astype(np.float32), dt)


def quant(x):
    """x [..., K] (the values of the input type, as any float array) -> (blocks uint8 [..., K/32, 16], scales uint8 [..., K/32])"""
    x = np.asarray(x, np.float64)
    assert x.shape[-1] % BLOCK == 0
    xb = x.reshape(x.shape[:-1] + (x.shape[-1] // BLOCK, BLOCK))
    bad = ~np.isfinite(xb).all(axis=-1)
    amax = np.where(bad, 0.0, np.abs(np.where(np.isfinite(xb), xb, 0.0)).max(axis=-1))
    zero = amax == 0
    floor_log2 = np.frexp(np.where(zero, 1.0, amax))[1] - 1                # amax = m 2^k, 0.5 <= m < 1: floor(log2) = k - 1
    s = np.clip(floor_log2 - 2, -127, 127)
    y = np.abs(np.where(np.isfinite(xb), xb, 0.0)) / np.ldexp(1.0, s)[..., None]
    m = np.zeros(xb.shape, np.uint8)
    for i, mid in enumerate(MIDPOINTS):                                    # code i + 1 is even for odd i: it wins its lower tie
        m += (y >= mid) if i % 2 else (y > mid)
    codes = np.where(bad[..., None], 0, m | (np.signbit(xb).astype(np.uint8) << 3)).astype(np.uint8)
    scales = np.where(bad, 255, np.where(zero, 0, s + 127)).astype(np.uint8)
    return pack(codes), scales


def random_packed(seed, shape, lo=119, hi=131):
    """random codes and scale bytes uniform in lo ... hi for weights [..., K]: (blocks [..., K/32, 16], scales [..., K/32])"""
    rng = np.random.default_rng(seed)
    nb = shape[-1] // BLOCK
    blocks = rng.integers(0, 256, size=tuple(shape[:-1]) + (nb, BLOCK // 2), dtype=np.uint8)
    scales = rng.integers(lo, hi + 1, size=tuple(shape[:-1]) + (nb,)).astype(np.uint8)
    return blocks, scales
