"""The yardstick of the tests of stochastic rounding with per-block scales: the contract of
include/ina_blk_sr.h replayed in numpy, written from the header's text.  The random words are those of
the WHOLE bucket (tests/_sr_ref.words: the scale has no part in them, and a block that starts off a
multiple of 4 has no e0 of its own), t is the value times its block's 2^k in float32, y is
tests/_sr_ref.y_of, and the clamps and the per-block flags are tests/_blk_ref.py's (the CPU oracle's
quantisers applied to y at k = 0, where rint(y * 1) is y itself).  Computed scales are
tests/_sr_ref.scale_for_sr per block.  Nothing here touches the GPU or the code under test."""
import numpy as np

from oracle import oracle as orc
from tests import _blk_ref as bref
from tests import _sr_ref as sref

F32 = np.float32


def _sub(sub: int, w: int) -> int:
    return (sub + w) & 0xFFFFFFFF


def scales_of(kblk, n: int, V: int) -> np.ndarray:
    """2^k of every element's block as float32; a given scale of -127 / -128 is read as -126."""
    k = np.maximum(np.asarray(kblk).astype(np.int32), -126)
    return np.ldexp(F32(1), np.repeat(k, V)[:n]).astype(F32)


def y_of(x, kblk, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0) -> np.ndarray:
    x = np.asarray(x).astype(F32)
    with np.errstate(all="ignore"):
        t = (x * scales_of(kblk, x.size, V)).astype(F32)
    return sref.y_of(t, sref.words(x.size, seed, step, sub, e0))


def _zeros(n: int, V: int) -> np.ndarray:
    return np.zeros((n + V - 1) // V, np.int8)


def quantize(x, kblk, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0) -> np.ndarray:
    y = y_of(x, kblk, V, seed, step, sub, e0)
    return bref.quantize_i32(y, _zeros(y.size, V), V)


def quantize_i16(x, kblk, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0):
    """(int16, one flag per block): one worker's summand of the int16 reduce."""
    y = y_of(x, kblk, V, seed, step, sub, e0)
    return bref.quantize_i16(y, _zeros(y.size, V), V)


def quantize_i16_wire(x, kblk, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0) -> np.ndarray:
    return orc.quantize_i16_wire(y_of(x, kblk, V, seed, step, sub, e0), 0)


def quantize_reduce(bufs, kblk, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0) -> np.ndarray:
    """int32: sum over w of q32_of(y_w), mod 2^32, worker w on stream sub + w."""
    return orc.sum_reduce_i32([quantize(b, kblk, V, seed, step, _sub(sub, w), e0) for w, b in enumerate(bufs)])


def quantize_reduce_i16(bufs, kblk, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0):
    """(int16, one flag per block): every summand saturated at int16, the sum saturated once; the flag is
    1 where a summand or the sum saturated or a y_w was NaN."""
    n = np.asarray(bufs[0]).size
    acc = np.zeros(n, np.int64)
    flags = np.zeros((n + V - 1) // V, np.uint8)
    for w, b in enumerate(bufs):
        q, f = quantize_i16(b, kblk, V, seed, step, _sub(sub, w), e0)
        acc += q.astype(np.int64)
        flags |= np.asarray(f, np.uint8)
    out = np.clip(acc, -32768, 32767)
    if n:
        flags |= np.maximum.reduceat((out != acc).astype(np.uint8), np.arange(0, n, V))
    return out.astype(np.int16), flags


def kblk_ref(xs, V: int, degree: int, bits: int) -> np.ndarray:
    """int8 [nblk]: ina_scale_for_sr's rule for the block's max |value| over the buffers, NaN ignored; a
    block holding +-inf gives -126."""
    d = np.abs(np.stack([np.asarray(x).astype(F32) for x in xs]))
    out = np.empty((d.shape[1] + V - 1) // V, np.int8)
    for s, sl in enumerate(bref.blocks(d.shape[1], V)):
        b = d[:, sl].ravel()
        out[s] = -126 if np.isinf(b).any() else sref.scale_for_sr(np.fmax.reduce(b, initial=F32(0)), degree, bits)
    return out
