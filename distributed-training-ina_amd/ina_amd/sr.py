"""Unbiased stochastic rounding for the quantisers (include/ina_sr.h): the stateless alternative to
error feedback (ina_amd.ef).

Each function is the ops / wire function of the same name with the rounding replaced:

    t = (x - base) * 2^k;   y = floor(t) + (u < t - floor(t));   q = the sibling's clamp of y

u is 24 bits of Philox4x32-10 under the key `seed` at the counter ((e0 + e) >> 2, step, sub), word
(e0 + e) & 3 -- a pure function of (seed, step, sub, element index), so every result can be replayed
(tests/_sr_ref.py) and depends on neither the grid nor the alignment.  E[q] = t where nothing clips;
where t is an integer q is the round-to-nearest result for every seed.  No bytes beyond the sibling's
move and nothing is kept between calls.

    k = sr.scale_for(amax, world, 16)                        # one more quantum of headroom than ops.scale_for
    w = sr.quantize_i16_wire(grad_bf16, k, seed, step=t, sub=rank)
    w = sr.quantize_i16_wire(grad[lo:hi], k, seed, step=t, sub=rank, e0=lo)   # that slice of the line above

x is float32, bfloat16 or float16; base is float32.  `step` is the training step, `sub` the stream within
it (ranks that share a seed must differ here, or they all round the same way), `e0` the offset of x in
its bucket, a multiple of 4.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops
from ._lib import check, load
from .ops import _fits, _ptr, _req, _req_grad, _same_device, _stream


def _params(seed: int, step: int, sub: int, e0: int) -> _lib.SrParams:
    for name, v, bits in (("seed", seed, 64), ("step", step, 32), ("sub", sub, 32), ("e0", e0, 64)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
        if not 0 <= v < 1 << bits:
            raise ValueError(f"{name} must be in [0, 2^{bits}), got {v}")
    if e0 % 4:
        raise ValueError(f"e0 must be a multiple of 4, got {e0}: a lane's 4 values share one Philox call")
    return _lib.SrParams(seed, e0, step, sub)


def _out(x: torch.Tensor, out, dtype):
    out = torch.empty(x.shape, dtype=dtype, device=x.device) if out is None else out
    _fits(out, x.numel())
    _req(out, dtype, "out")
    _same_device(x, out)
    return out


def quantize(x: torch.Tensor, k: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0,
             base: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.quantize of x - base, rounded stochastically: int32."""
    xt = _req_grad(x, "x")
    prm = _params(seed, step, sub, e0)
    ops._base_arg(base, x.numel(), x, "x")
    out = _out(x, out, torch.int32)
    if xt:
        rc = load().ina_quantize_sr_x16_i32(x.data_ptr(), xt, _ptr(base), out.data_ptr(), x.numel(), k,
                                            C.byref(prm), _stream(x))
    else:
        rc = load().ina_quantize_sr_f32_i32(x.data_ptr(), _ptr(base), out.data_ptr(), x.numel(), k, C.byref(prm),
                                            _stream(x))
    check(rc, "sr.quantize")
    return out


def quantize_i16(x: torch.Tensor, k: int, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0,
                 base: torch.Tensor | None = None, out=None, overflow=None):
    """ops.quantize_i16 of x - base, rounded stochastically: (out int16, overflow), one flag per slot
    of V values (a slot is V values of x: with e0 != 0 the caller keeps lo a multiple of V)."""
    xt = _req_grad(x, "x")
    prm = _params(seed, step, sub, e0)
    if V <= 0:
        raise ValueError("V must be > 0")
    ops._base_arg(base, x.numel(), x, "x")
    out = _out(x, out, torch.int16)
    nslot = (x.numel() + V - 1) // V
    overflow = torch.empty(nslot, dtype=torch.uint8, device=x.device) if overflow is None else overflow
    _fits(overflow, nslot, "overflow")
    _req(overflow, torch.uint8, "overflow")
    _same_device(x, overflow)
    if xt:
        rc = load().ina_quantize_sr_x16_i16_sat(x.data_ptr(), xt, _ptr(base), out.data_ptr(), x.numel(), k, V,
                                                overflow.data_ptr(), C.byref(prm), _stream(x))
    else:
        rc = load().ina_quantize_sr_f32_i16_sat(x.data_ptr(), _ptr(base), out.data_ptr(), x.numel(), k, V,
                                                overflow.data_ptr(), C.byref(prm), _stream(x))
    check(rc, "sr.quantize_i16")
    return out, overflow


def quantize_i16_wire(x: torch.Tensor, k: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """wire.quantize rounded stochastically: the int32 wire words q16 + (saturated << 22) of
    dist.ShardedAggregator(wire="i16", rounding="stochastic")."""
    xt = _req_grad(x, "x")
    prm = _params(seed, step, sub, e0)
    out = _out(x, out, torch.int32)
    if xt:
        rc = load().ina_quantize_sr_x16_i16_wire(x.data_ptr(), xt, out.data_ptr(), x.numel(), k, C.byref(prm),
                                                 _stream(x))
    else:
        rc = load().ina_quantize_sr_f32_i16_wire(x.data_ptr(), out.data_ptr(), x.numel(), k, C.byref(prm), _stream(x))
    check(rc, "sr.quantize_i16_wire")
    return out


def scale_for(amax: float, W: int, bits: int) -> int:
    """ops.scale_for with a whole quantum of rounding a value: the largest k in [-126, 127] with
    W * (amax * 2^k + 1) <= 2^(bits-1) - 1, so no W-way sum of stochastically rounded values clips."""
    k = C.c_int(0)
    check(load().ina_scale_for_sr(float(amax), int(W), int(bits), C.byref(k)), "sr.scale_for")
    return k.value
