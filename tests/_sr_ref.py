"""The yardstick of the stochastic-rounding tests: a numpy replay of the contract of include/ina_sr.h,
written from the header's text.  Philox4x32-10 in uint64 arithmetic, u, y in explicit float32 steps,
the existing CPU oracle's clamps where it has them (its quantisers applied to y at k = 0, where
rint(y * 1) is y itself), and ina_scale_for_sr in exact rationals.  Nothing here touches the GPU or a
stochastic-rounding entry point."""
from fractions import Fraction

import numpy as np

from oracle import oracle as orc

F32 = np.float32
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Ten rounds over arrays (or scalars) of counters: the four output words as uint32 arrays."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]           # < 2^64: no wrap
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & MASK]
    return [v.astype(np.uint32) for v in c]


def words(n: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0) -> np.ndarray:
    """The word of each of n elements: counter ((e0 + e) >> 2, step, sub), output word (e0 + e) & 3."""
    assert e0 % 4 == 0
    g = np.arange(n, dtype=np.uint64) + np.uint64(e0)
    idx = g >> np.uint64(2)
    out = philox4x32_10(idx & MASK, idx >> np.uint64(32), step, sub, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(out, axis=1)[np.arange(n), (g & np.uint64(3)).astype(np.int64)]


def uniform(w: np.ndarray) -> np.ndarray:
    """u = float(word >> 8) * 2^-24: exact in float32, in [0, 1)."""
    return ((w >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)


def t_of(x, k: int, base=None) -> np.ndarray:
    """t = (x - base) * 2^k in float32, one rounding per operation; x may be any float dtype that
    widens exactly."""
    with np.errstate(all="ignore"):
        d = np.asarray(x).astype(F32)
        if base is not None:
            d = (d - np.asarray(base, F32)).astype(F32)
        return (d * np.ldexp(F32(1), int(k)).astype(F32)).astype(F32)


def y_of(t: np.ndarray, w: np.ndarray) -> np.ndarray:
    """y = floor(t) + (u < t - floor(t)): NaN stays NaN, +-inf stays +-inf (p is NaN there)."""
    with np.errstate(all="ignore"):
        f = np.floor(t).astype(F32)
        p = (t - f).astype(F32)
        return (f + np.where(uniform(w) < p, F32(1), F32(0))).astype(F32)


def _y(x, k, seed, step, sub, e0, base):
    t = t_of(x, k, base)
    return y_of(t, words(t.size, seed, step, sub, e0))


def quantize(x, k: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0, base=None) -> np.ndarray:
    """int32: the oracle's clamp (NaN -> 0, saturation at the int32 limits) of y."""
    return orc.quantize_i32(_y(x, k, seed, step, sub, e0, base), 0)


def quantize_i16(x, k: int, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0, base=None):
    """(int16, one flag per slot of V values): the oracle's saturating clamp and flags of y."""
    return orc.quantize_i16_sat(_y(x, k, seed, step, sub, e0, base), 0, V)


def quantize_i16_wire(x, k: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0) -> np.ndarray:
    """The int32 wire words q16 + (sat << 22) of y."""
    return orc.quantize_i16_wire(_y(x, k, seed, step, sub, e0, None), 0)


def scale_for_sr(amax, W: int, bits: int) -> int:
    """The largest k in [-126, 127] with W * (amax * 2^k + 1) <= 2^(bits-1) - 1 in exact rationals
    (-126 if there is none; 127 for amax = 0)."""
    a = Fraction(float(F32(amax)))
    top = Fraction(2 ** (bits - 1) - 1)
    assert top / W - 1 > 0
    for k in range(127, -127, -1):
        if W * (a * Fraction(2) ** k + 1) <= top:
            return k
    return -126
