"""The int16 wire of a sharded bucket for any gradient dtype (include/ina.h, include/ina_shard_blk.h,
include/ina_shard_x16.h), as ina_amd.blk is for block scales.

quantize / quantize_blk take a float32, bfloat16 or float16 bucket; finish / finish_blk write y as
float32, bfloat16 or float16.  Whatever is float32 goes to the ops function of the same arguments
unchanged (ops.quantize_i16_wire, ops.quantize_i16_wire_blk, ops.i16_wire_finish,
ops.i16_wire_finish_blk, which keep refusing 16-bit tensors).  A 16-bit bucket is read as it is: its
wire words are bit for bit the float32 ones on the widened (.float()) bucket, without the widening
pass and its twice as large temporary.  A 16-bit y is the float32 y rounded once to nearest even, bit
for bit ops.dequantize / blk.dequantize of out16 into that dtype; out16 and the flags do not depend on
y's dtype.  No CPU fallback.

    w = wire.quantize_blk(grad_bf16, kblk, V)                         # then an int32 SUM over ranks
    s16, g, ovf = wire.finish_blk(w, kblk, V, dtype=torch.bfloat16)
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import check, load
from .ops import _X16, _blk_scales_arg, _blk_v, _fits, _req, _req_grad, _same_device, _stream


def _is16(t) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype in _X16


def _wire_out(x: torch.Tensor, out):
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device) if out is None else out
    _fits(out, x.numel())
    _req(out, torch.int32, "out")
    _same_device(x, out)
    return out


def quantize(x: torch.Tensor, k: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.quantize_i16_wire for a float32, bfloat16 or float16 bucket."""
    if not _is16(x):
        return ops.quantize_i16_wire(x, k, out)
    xt = _req_grad(x, "x")
    out = _wire_out(x, out)
    check(load().ina_quantize_x16_i16_wire(x.data_ptr(), xt, out.data_ptr(), x.numel(), k, _stream(x)),
          "quantize_i16_wire")
    return out


def quantize_blk(x: torch.Tensor, kblk: torch.Tensor, V: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.quantize_i16_wire_blk for a float32, bfloat16 or float16 bucket."""
    if not _is16(x):
        return ops.quantize_i16_wire_blk(x, kblk, V, out)
    V = _blk_v(V)
    xt = _req_grad(x, "x")
    kblk = _blk_scales_arg(kblk, (x.numel() + V - 1) // V, x, given=True)
    out = _wire_out(x, out)
    check(load().ina_quantize_blk_x16_i16_wire(x.data_ptr(), xt, kblk.data_ptr(), V, out.data_ptr(), x.numel(),
                                               _stream(x)), "quantize_i16_wire_blk")
    return out


def _y16(y, dtype) -> bool:
    """Whether a finish writes a 16-bit y: the dtype of y decides, `dtype` only when y is None."""
    if y is not None:
        if not isinstance(y, torch.Tensor):
            raise TypeError("y must be a torch.Tensor")
        if y.dtype != torch.float32 and y.dtype not in _X16:
            raise TypeError(f"y must be float32, bfloat16 or float16, got {y.dtype}")
        return y.dtype in _X16
    if dtype != torch.float32 and dtype not in _X16:
        raise TypeError(f"dtype must be float32, bfloat16 or float16, got {dtype}")
    return dtype in _X16


def _finish_outs(wire_sum, V, out16, y, overflow, want_out16, want_y, dtype):
    """The 16-bit finishes' outputs, allocated where not given and checked by name: (out16, y, overflow,
    y's pointer, its type code).  With y neither given nor wanted the type code is `dtype`'s."""
    _req(wire_sum, torch.int32, "wire_sum")
    n, dev = wire_sum.numel(), wire_sum.device
    nslot = (n + V - 1) // V
    if out16 is None and want_out16:
        out16 = torch.empty(n, dtype=torch.int16, device=dev)
    if y is None and want_y:
        y = torch.empty(n, dtype=dtype, device=dev)
    overflow = torch.empty(nslot, dtype=torch.uint8, device=dev) if overflow is None else overflow
    ydt = y.dtype if y is not None else dtype
    for t, dt, cnt, name in ((out16, torch.int16, n, "out16"), (y, ydt, n, "y"),
                             (overflow, torch.uint8, nslot, "overflow")):
        if t is not None:
            _fits(t, cnt, name)
            _req(t, dt, name)
            _same_device(wire_sum, t)
    return out16, y, overflow, (y.data_ptr() if y is not None else None), _X16[ydt]


def finish(wire_sum: torch.Tensor, k: int, V: int, out16=None, y=None, overflow=None, want_out16: bool = True,
           want_y: bool = True, dtype: torch.dtype = torch.float32):
    """ops.i16_wire_finish with y as float32, bfloat16 or float16: (out16, y, overflow)."""
    if not _y16(y, dtype):
        return ops.i16_wire_finish(wire_sum, k, V, out16, y, overflow, want_out16, want_y)
    if V <= 0:
        raise ValueError("V must be > 0")
    out16, y, overflow, yp, yt = _finish_outs(wire_sum, V, out16, y, overflow, want_out16, want_y, dtype)
    check(load().ina_i16_wire_finish_x16(wire_sum.data_ptr(), wire_sum.numel(), k, V,
                                         out16.data_ptr() if out16 is not None else None, yp, yt,
                                         overflow.data_ptr(), _stream(wire_sum)), "i16_wire_finish")
    return out16, y, overflow


def finish_blk(wire_sum: torch.Tensor, kblk: torch.Tensor, V: int, out16=None, y=None, overflow=None,
               want_out16: bool = True, want_y: bool = True, dtype: torch.dtype = torch.float32):
    """ops.i16_wire_finish_blk with y as float32, bfloat16 or float16: (out16, y, overflow)."""
    if not _y16(y, dtype):
        return ops.i16_wire_finish_blk(wire_sum, kblk, V, out16, y, overflow, want_out16, want_y)
    V = _blk_v(V)
    _req(wire_sum, torch.int32, "wire_sum")
    kblk = _blk_scales_arg(kblk, (wire_sum.numel() + V - 1) // V, wire_sum, given=True)
    out16, y, overflow, yp, yt = _finish_outs(wire_sum, V, out16, y, overflow, want_out16, want_y, dtype)
    check(load().ina_i16_wire_finish_blk_x16(wire_sum.data_ptr(), wire_sum.numel(), kblk.data_ptr(), V,
                                             out16.data_ptr() if out16 is not None else None, yp, yt,
                                             overflow.data_ptr(), _stream(wire_sum)), "i16_wire_finish_blk")
    return out16, y, overflow
