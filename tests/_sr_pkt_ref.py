"""The yardstick of the stochastic-rounding packet tests: a numpy replay of the contract of
include/ina_pkt_sr.h, written from the header's text on top of tests/_sr_ref.py (the Philox replay
and the rounding step) and the CPU oracle (the int32 clamp and the NGA pack).  Nothing here touches
the GPU or a stochastic-rounding entry point."""
from fractions import Fraction

import numpy as np

from oracle import oracle as orc
from tests import _sr_ref as S

F32 = np.float32
NUM_SLOTS = 16384


def scales_read(kblk) -> np.ndarray:
    """ina_blk.h's reading of given scales: -127 / -128 read as -126."""
    return np.maximum(np.asarray(kblk).astype(np.int64), -126)


def quantize(x, k, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0, base=None) -> np.ndarray:
    """One worker's int32 words.  k an int: _sr_ref.quantize.  k an array of per-packet scales:
    element e is rounded on t = d * 2^k[e / V], its word still that of element e0 + e."""
    x = np.asarray(x, F32)
    if np.ndim(k) == 0:
        return S.quantize(x, int(k), seed, step, sub, e0, base)
    kk = np.repeat(scales_read(k), V)[:x.size]
    with np.errstate(all="ignore"):
        d = x if base is None else (x - np.asarray(base, F32)).astype(F32)
        t = (d * np.ldexp(F32(1), kk).astype(F32)).astype(F32)
    return orc.quantize_i32(S.y_of(t, S.words(x.size, seed, step, sub, e0)), 0)


def workers(xs, k, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0, base=None):
    """Worker w of a multi-worker call draws from stream sub + w (mod 2^32)."""
    return [quantize(x, k, V, seed, step, (sub + w) & 0xFFFFFFFF, e0, base) for w, x in enumerate(xs)]


def scale_for_sr(amax, W: int, bits: int) -> int:
    """_sr_ref.scale_for_sr, found by bisection: its predicate W * (amax * 2^k + 1) <= 2^(bits-1) - 1, in
    the same exact rationals, only falls as k grows, so the largest k that holds is the same k
    (tests/test_pkt_sr_api.py compares the two)."""
    a, top = Fraction(float(F32(amax))), Fraction(2 ** (bits - 1) - 1)
    assert top / W - 1 > 0

    def holds(k):
        return W * (a * Fraction(2) ** k + 1) <= top
    if holds(127):
        return 127
    lo, hi = -126, 127                                     # holds(hi) is false; lo is the answer if nothing holds
    if not holds(lo):
        return -126
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if holds(mid) else (lo, mid)
    return lo


def block_scales(xs, V: int, degree: int, bits: int = 32, base=None) -> np.ndarray:
    """_sr_ref.scale_for_sr of each block's max |x_w - base| over the workers: NaN skipped, a block
    holding inf -126, all zero / all NaN 127."""
    with np.errstate(all="ignore"):
        d = [np.abs(np.asarray(x, F32) if base is None else (np.asarray(x, F32) - np.asarray(base, F32)).astype(F32))
             for x in xs]
    a = np.fmax.reduce([np.where(np.isnan(v), F32(0), v) for v in d])
    n = a.size
    out = np.empty((n + V - 1) // V, np.int8)
    for b in range(out.size):
        m = a[b * V:(b + 1) * V].max()
        out[b] = -126 if np.isinf(m) else scale_for_sr(m, degree, bits)
    return out


def rows(q, V: int, bitmap: int, count: int, seq0: int, stride=None, switch_id: int = 1, num_slots: int = NUM_SLOTS):
    """The packed rows of the plain pack of q (the oracle's)."""
    return orc.pack_nga(q, V, bitmap, count, switch_id, seq0, num_slots=num_slots, stride=stride)


def split_of(r, V: int):
    """Packed rows as split rows: 16-byte header rows (byte 15 zero) and 4V-byte payload rows."""
    hdr = np.zeros((len(r), 16), np.uint8)
    hdr[:, :15] = r[:, :15]
    return hdr, np.ascontiguousarray(r[:, 15:15 + 4 * V])


def desc_of(r):
    return np.ascontiguousarray(r[:, 4:12]).view(np.int64).ravel()


def ps_update(local, qs, k, V: int, weight_step: float) -> np.ndarray:
    """The PS update as the unfused fp32 sequence local + (float(sum) * 2^-k) * float(weight_step), the W
    words summed mod 2^32; k an int or per-packet scales."""
    local = np.asarray(local, F32)
    s = np.zeros(local.size, np.uint32)
    for q in qs:
        s = s + np.asarray(q, np.int32).view(np.uint32)        # uint32: wraps
    kk = np.full(local.size, int(k), np.int64) if np.ndim(k) == 0 else np.repeat(scales_read(k), V)[:local.size]
    inv = np.ldexp(F32(1), -kk).astype(F32)
    y = (s.view(np.int32).astype(F32) * inv).astype(F32)
    return (local + (y * F32(weight_step)).astype(F32)).astype(F32)


def bias_case(seed: int, rounding: str = "stochastic", W: int = 4, n: int = 65536, k: int = 9):
    """The end-to-end bias case: every value 0.3f * 2^-9 at k = 9, worker w on stream w.  Returns the
    sum over the workers of each element's word (int64)."""
    x = np.full(n, F32(0.3) * F32(2.0 ** -9), F32)
    if rounding == "nearest":
        return sum(orc.quantize_i32(x, k).astype(np.int64) for _ in range(W))
    return sum(q.astype(np.int64) for q in workers([x] * W, k, 256, seed))
