"""The yardstick of the stochastic fused quantise + reduce tests: the contract of include/ina_reduce_sr.h
replayed in numpy, written from the header's text.  Worker w's summand is tests/_sr_ref.py's quantiser on
stream sub + w (mod 2^32); the int32 sum is the CPU oracle's wrapping sum; the int16 sum is taken in int64
and clamped once, and a slot's flag is the OR of the workers' flags with the final clamp.  Nothing here
touches the GPU or the code under test."""
import numpy as np

from oracle import oracle as orc
from tests import _sr_ref as sref


def _sub(sub: int, w: int) -> int:
    return (sub + w) & 0xFFFFFFFF


def quantize_reduce(bufs, k: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0) -> np.ndarray:
    """int32: sum over w of q32_of(y_w), mod 2^32."""
    return orc.sum_reduce_i32([sref.quantize(b, k, seed, step, _sub(sub, w), e0) for w, b in enumerate(bufs)])


def quantize_reduce_i16(bufs, k: int, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0):
    """(int16, one flag per slot of V values): every summand saturated at int16, the sum saturated once;
    the flag is 1 where a summand or the sum saturated or a y_w was NaN."""
    n = np.asarray(bufs[0]).size
    nslot = -(-n // V)
    acc = np.zeros(n, np.int64)
    flags = np.zeros(nslot, np.uint8)
    for w, b in enumerate(bufs):
        q, f = sref.quantize_i16(b, k, V, seed, step, _sub(sub, w), e0)
        acc += q.astype(np.int64)
        flags |= np.asarray(f, np.uint8)
    out = np.clip(acc, -32768, 32767)
    clipped = out != acc
    if n:
        flags |= np.maximum.reduceat(clipped.astype(np.uint8), np.arange(0, n, V))
    return out.astype(np.int16), flags
