"""The yardstick of the 4-bit wire's tests: the contract of include/ina_i4.h in numpy, on top of the byte wire's
(tests/_i8_ref.py).  Nothing here touches the GPU or the code under test."""
from fractions import Fraction

import numpy as np

from tests import _i8_ref as ref8

F32 = np.float32
dequantize = ref8.dequantize


def scale_for(absmax) -> int:
    """The largest k in [-126, 127] with absmax * 2^k + 1/2 <= 7, searched in exact arithmetic."""
    a = Fraction(float(absmax))
    return next((k for k in range(127, -126, -1) if a * Fraction(2) ** k + Fraction(1, 2) <= 7), -126)


def block_scales(xs, V, rotate=None, **key) -> np.ndarray:
    a = np.abs(np.stack([ref8.rotated(x, V, rotate, **key) for x in xs])).reshape(len(xs), -1, V)
    amax = np.fmax.reduce(np.fmax.reduce(a, axis=2, initial=F32(0)), axis=0)       # NaN ignored
    return np.array([-126 if np.isinf(m) else scale_for(m) for m in amax], np.int8)


def pack(q) -> np.ndarray:
    """Value e in byte e / 2: even e in the low nibble, odd e in the high one."""
    u = np.asarray(q).astype(np.uint8) & 15
    return u[0::2] | (u[1::2] << 4)


def unpack(b) -> np.ndarray:
    b = np.asarray(b, np.uint8)
    u = np.stack([b & 15, b >> 4], axis=-1).reshape(*b.shape[:-1], -1).astype(np.int16)
    return u - 16 * (u > 7)


def quantize(x, kblk, V, rotate=None, **key):
    """(packed nibbles, one flag per block: clamped or NaN)."""
    s = np.repeat(np.ldexp(F32(1), np.maximum(np.asarray(kblk, np.int32), -126)).astype(F32), V)
    with np.errstate(all="ignore"):
        y = np.rint((ref8.rotated(x, V, rotate, **key) * s).astype(F32))
    c = np.clip(y, -7, 7)
    flags = ((c != y) | np.isnan(y)).reshape(-1, V).any(1).astype(np.uint8)
    return pack(np.where(np.isnan(y), 0, c).astype(np.int8)), flags


def sum_slices(parts) -> np.ndarray:
    return unpack(np.stack(parts)).astype(np.int32).sum(0).astype(np.int16)


def requant(parts, V):
    """(q8, shift) from the exact sums: np.rint is round half to even and S / 2^sh is exact."""
    S = sum_slices(parts).astype(np.int64)
    sh = (np.rint(np.abs(S).reshape(-1, V).max(1)[:, None] / 2.0 ** np.arange(8)) > 127).sum(1)    # the first that fits
    return np.rint(S / 2.0 ** np.repeat(sh, V)).astype(np.int8), sh.astype(np.uint8)
