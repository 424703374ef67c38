"""The contract of include/ina_i8_sr.h in numpy, written from the header's text on top of tests/_sr_ref.py (Philox,
y_of) and tests/_i8_ref.py (rotated), with exact integers for the requantiser.  Nothing here touches the GPU."""
from fractions import Fraction

import numpy as np

from tests import _i8_ref as i8ref
from tests import _sr_ref as srref

F32 = np.float32


def scale_for_sr(absmax) -> int:
    """The largest k in [-126, 127] with absmax * 2^k + 1 <= 127, searched in exact arithmetic."""
    a = Fraction(float(absmax))
    return next((k for k in range(127, -126, -1) if a * Fraction(2) ** k + 1 <= 127), -126)


def block_scales(xs, V, rotate=None, **key) -> np.ndarray:
    a = np.abs(np.stack([i8ref.rotated(x, V, rotate, **key) for x in xs])).reshape(len(xs), -1, V)
    amax = np.fmax.reduce(np.fmax.reduce(a, axis=2, initial=F32(0)), axis=0)       # NaN ignored
    return np.array([-126 if np.isinf(m) else scale_for_sr(m) for m in amax], np.int8)


def quantize(x, kblk, V, seed, rotate=None, step=0, sub=0, e0=0, rot_sub=0, rot_e0=0):
    """(int8 q, one flag per block: clamped or NaN): the clamp of ina_sr.h's y of t = r * 2^kblk."""
    s = np.repeat(np.ldexp(F32(1), np.maximum(np.asarray(kblk, np.int32), -126)).astype(F32), V)
    with np.errstate(all="ignore"):
        t = (i8ref.rotated(x, V, rotate, step, rot_sub, rot_e0) * s).astype(F32)
        y = srref.y_of(t, srref.words(t.size, seed, step, sub, e0))
    c = np.clip(y, -127, 127)
    flags = ((c != y) | np.isnan(y)).reshape(-1, V).any(1).astype(np.uint8)
    return np.where(np.isnan(y), 0, c).astype(np.int8), flags


def random_bytes(n, seed, step=0, sub=0, e0=0) -> np.ndarray:
    """byte g & 3 of word (g >> 2) & 3 of the call at counter (g >> 4, step, sub), g = e0 + e."""
    assert e0 % 16 == 0
    g = np.arange(n, dtype=np.uint64) + np.uint64(e0)
    idx = g >> np.uint64(4)
    out = srref.philox4x32_10(idx & srref.MASK, idx >> np.uint64(32), step, sub, seed & 0xFFFFFFFF, seed >> 32)
    w = np.stack(out, axis=1)[np.arange(n), ((g >> np.uint64(2)) & np.uint64(3)).astype(np.int64)].astype(np.int64)
    return (w >> (8 * (g & np.uint64(3)).astype(np.int64))) & 0xFF


def requant(parts, V, seed, step=0, sub=0, e0=0):
    """(q8, shift): exact sums, the smallest sh with A <= 127 << sh, q8 = (S + (byte & (2^sh - 1))) >> sh."""
    S = np.asarray(parts).astype(np.int64).sum(0)
    sh = (np.abs(S).reshape(-1, V).max(1)[:, None] > (127 << np.arange(8))).sum(1)
    shv = np.repeat(sh, V)
    q = (S + (random_bytes(S.size, seed, step, sub, e0) & ((1 << shv) - 1))) >> shv     # >> on int64 is arithmetic
    assert np.abs(q).max(initial=0) <= 127
    return q.astype(np.int8), sh.astype(np.uint8)
