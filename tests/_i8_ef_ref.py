"""The yardstick of the byte wire's error-feedback tests: the contract of include/ina_i8_ef.h in numpy float32, on
top of tests/_i8_ref.py and tests/_rot_ref.py.  Nothing here touches the GPU or the code under test."""
import numpy as np

from tests import _i8_ref as ref

F32, rref = ref.F32, ref.rref


def _v(x, resid):
    with np.errstate(all="ignore"):
        return (np.asarray(x).astype(F32) + np.asarray(resid, F32)).astype(F32)


def block_scales(xs, resids, V, rotate=None, **key) -> np.ndarray:
    return ref.block_scales([_v(x, r) for x, r in zip(xs, resids)], V, rotate, **key)


def quantize(x, resid, kblk, V, rotate=None, **key):
    """(int8 q, flags, resid', u before the last guard)."""
    v = _v(x, resid)
    q, flags = ref.quantize(v, kblk, V, rotate, **key)
    inv = np.repeat(np.ldexp(F32(1), -np.maximum(np.asarray(kblk, np.int32), -126)).astype(F32), V)
    with np.errstate(all="ignore"):
        r = ref.rotated(v, V, rotate, **key)
        d = np.where(np.isfinite(r), (r - (q.astype(F32) * inv).astype(F32)).astype(F32), F32(0))
        u = d if rotate is None else rref.inverse(d, V, rref.signs(v.size, rotate, **key))
    return q, flags, np.where(np.isfinite(u), u, F32(0)).astype(F32), u
