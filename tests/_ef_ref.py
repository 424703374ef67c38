"""The yardstick of the error-feedback tests (include/ina_ef.h): the existing CPU oracle's quantiser
applied to v = (x - base) + r, and the three numpy float32 operations around it.  Per block it is
called once per block with that block's k, as tests/_blk_ref.py does.  Nothing here touches the GPU
or an error-feedback entry point."""
import numpy as np

from oracle import oracle as orc
from tests import _blk_ref as ref

F32 = np.float32


def v_of(x, r, base=None) -> np.ndarray:
    """v = (x - base) + r in float32; x may be any float dtype that widens exactly."""
    with np.errstate(all="ignore"):
        d = np.asarray(x).astype(F32)
        if base is not None:
            d = (d - np.asarray(base, F32)).astype(F32)
        return (d + np.asarray(r, F32)).astype(F32)


def carry(v, q, k: int) -> np.ndarray:
    """r' = isfinite(v) ? v - float(q) * 2^-k : +0, 2^-k exact (k = 127: the subnormal)."""
    with np.errstate(all="ignore"):
        y = (q.astype(F32) * np.ldexp(F32(1), -int(k)).astype(F32)).astype(F32)
        return np.where(np.isfinite(v), (v - y).astype(F32), F32(0)).astype(F32)


def quantize(x, r, k: int, base=None):
    """(q int32, r')"""
    v = v_of(x, r, base)
    q = orc.quantize_i32(v, k)
    return q, carry(v, q, k)


def quantize_i16(x, r, k: int, V: int, base=None):
    """(q int16, one flag per slot of V values, r')"""
    v = v_of(x, r, base)
    q, f = orc.quantize_i16_sat(v, k, V)
    return q, f, carry(v, q, k)


def block_scales(xs, rs, V: int, degree: int, bits: int, base=None) -> np.ndarray:
    """ina_scale_for of each block's max |v| over the workers."""
    return ref.kblk_ref([v_of(x, r, base) for x, r in zip(xs, rs)], V, degree, bits)


def quantize_blk(x, r, kblk, V: int, base=None):
    v = v_of(x, r, base)
    q = ref.quantize_i32(v, kblk, V)
    rn = np.concatenate([carry(v[sl], q[sl], ref.keff(kblk[s])) for s, sl in enumerate(ref.blocks(v.size, V))])
    return q, rn


def quantize_i16_blk(x, r, kblk, V: int, base=None):
    v = v_of(x, r, base)
    q, f = ref.quantize_i16(v, kblk, V)
    rn = np.concatenate([carry(v[sl], q[sl], ref.keff(kblk[s])) for s, sl in enumerate(ref.blocks(v.size, V))])
    return q, f, rn


def bits(a) -> np.ndarray:
    """A float32 array as its bit patterns (NaN payloads and the sign of zero compare)."""
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)
