"""The yardstick of the rotation tests: the contract of include/ina_rot.h in numpy, written from the header's
text -- the signs, a float32 replay (every add and multiply rounded to float32, in the contract's stage order)
and a float64 version of the same transforms.  The quantisers, the scales and the plain decode are the block
yardstick's (tests/_blk_ref.py: the CPU oracle per block).  Nothing here touches the GPU or the code under
test."""
import numpy as np

from tests import _blk_ref as bref
from tests._sr_ref import MASK, philox4x32_10

F32 = np.float32


def signs(n: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0) -> np.ndarray:
    """sigma(e) as +-1 (int8): bit (g & 31) of word (g >> 5) & 3 of Philox at counter (g >> 7, step, sub)."""
    g = np.arange(n, dtype=np.uint64) + np.uint64(e0)
    idx = g >> np.uint64(7)
    w = np.stack(philox4x32_10(idx & MASK, idx >> np.uint64(32), step, sub, seed & 0xFFFFFFFF, seed >> 32), axis=1)
    word = w[np.arange(n), ((g >> np.uint64(5)) & np.uint64(3)).astype(np.int64)]
    bit = (word >> (g & np.uint64(31)).astype(np.uint32)) & np.uint32(1)
    return np.where(bit == 1, -1, 1).astype(np.int8)


def _stages(t: np.ndarray, V: int) -> np.ndarray:
    """The m stages in the contract's order, in t's dtype; t: [..., n], n a multiple of V."""
    shape, dt = t.shape, t.dtype
    for i in range(V.bit_length() - 1):
        h = 1 << i
        p = t.reshape(-1, 2, h)
        with np.errstate(all="ignore"):
            t = np.stack([(p[:, 0] + p[:, 1]).astype(dt), (p[:, 0] - p[:, 1]).astype(dt)], axis=1)
    return t.reshape(shape)


def forward(x, V: int, sg, dtype=F32) -> np.ndarray:
    """r = stages(sigma * x) * 2^-ceil(m/2); x is widened to float32 first (exact)."""
    m = V.bit_length() - 1
    t = np.asarray(x).astype(F32).astype(dtype) * sg.astype(dtype)
    with np.errstate(all="ignore"):
        return (_stages(t, V) * dtype(2.0 ** -((m + 1) // 2))).astype(dtype)


def inverse(y, V: int, sg, dtype=F32) -> np.ndarray:
    """xhat = sigma * (stages(y) * 2^-floor(m/2))."""
    m = V.bit_length() - 1
    with np.errstate(all="ignore"):
        u = (_stages(np.asarray(y).astype(dtype), V) * dtype(2.0 ** -(m // 2))).astype(dtype)
    return u * sg.astype(dtype)


def quantize_reduce(bufs, V: int, seed: int, kblk=None, degree=None, bits: int = 32, step=0, sub=0, e0=0):
    """(q, flags or None, kblk): the float32 replay of both fused calls; kblk=None is AUTO."""
    sg = signs(np.asarray(bufs[0]).size, seed, step, sub, e0)
    rs = [forward(b, V, sg) for b in bufs]
    if kblk is None:
        kblk = bref.kblk_ref(rs, V, len(bufs) if degree is None else degree, bits)
    if bits == 32:
        return bref.quantize_reduce_i32(rs, kblk, V), None, kblk
    q, flags = bref.quantize_reduce_i16(rs, kblk, V)
    return q, flags, kblk


def dequantize(s, kblk, V: int, seed: int, step=0, sub=0, e0=0, dtype=F32) -> np.ndarray:
    """The decode: float(s) * 2^-k per block (exact in either dtype), then the inverse rotation."""
    return inverse(bref.dequantize(np.asarray(s), kblk, V), V, signs(np.asarray(s).size, seed, step, sub, e0), dtype)
