"""The yardstick of the 8-bit wire's tests: the contract of include/ina_i8.h in numpy, on top of the rotation's
(tests/_rot_ref.py) -- the scale rule, the byte quantiser and the exact slice sum.  Nothing here touches the
GPU or the code under test."""
from fractions import Fraction

import numpy as np

from tests import _rot_ref as rref

F32 = np.float32


def scale_for(absmax) -> int:
    """The largest k in [-126, 127] with absmax * 2^k + 1/2 <= 127, searched in exact arithmetic."""
    a = Fraction(float(absmax))
    return next((k for k in range(127, -126, -1) if a * Fraction(2) ** k + Fraction(1, 2) <= 127), -126)


def rotated(x, V, rotate=None, step=0, sub=0, e0=0, dtype=F32):
    """r of the contract: the widened x, or its forward rotation under the seed `rotate`."""
    x = np.asarray(x).astype(F32)
    return x.astype(dtype) if rotate is None else rref.forward(x, V, rref.signs(x.size, rotate, step, sub, e0), dtype)


def block_scales(xs, V, rotate=None, **key) -> np.ndarray:
    a = np.abs(np.stack([rotated(x, V, rotate, **key) for x in xs])).reshape(len(xs), -1, V)
    amax = np.fmax.reduce(np.fmax.reduce(a, axis=2, initial=F32(0)), axis=0)       # NaN ignored
    return np.array([-126 if np.isinf(m) else scale_for(m) for m in amax], np.int8)


def quantize(x, kblk, V, rotate=None, **key):
    """(int8 q, one flag per block: clamped or NaN)."""
    s = np.repeat(np.ldexp(F32(1), np.maximum(np.asarray(kblk, np.int32), -126)).astype(F32), V)
    with np.errstate(all="ignore"):
        y = np.rint((rotated(x, V, rotate, **key) * s).astype(F32))
    c = np.clip(y, -127, 127)
    flags = ((c != y) | np.isnan(y)).reshape(-1, V).any(1).astype(np.uint8)
    return np.where(np.isnan(y), 0, c).astype(np.int8), flags


def sum_slices(parts) -> np.ndarray:
    return np.sum(np.stack(parts).astype(np.int32), axis=0).astype(np.int16)


def requant(parts, V):
    """(q8, shift) of include/ina_i8_gather.h from exact sums: np.rint is round half to even, and S / 2^sh is exact."""
    S = np.asarray(parts).astype(np.int64).sum(0)
    A = np.abs(S).reshape(-1, V).max(1)
    sh = (np.rint(A[:, None] / 2.0 ** np.arange(8)) > 127).sum(1)      # rne is monotone in sh: the first that fits
    return np.rint(S / 2.0 ** np.repeat(sh, V)).astype(np.int8), sh.astype(np.uint8)


def dequantize(s16, kblk, V, rotate=None, dtype=F32, **key) -> np.ndarray:
    """The existing decodes on the int16 sums."""
    if rotate is None:
        return rref.bref.dequantize(np.asarray(s16), kblk, V).astype(dtype)
    return rref.dequantize(s16, kblk, V, rotate, dtype=dtype, **key)
