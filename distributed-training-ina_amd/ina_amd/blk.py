"""Per-block scales for any gradient dtype (include/ina_blk.h, include/ina_x16_blk.h).

Each function takes the arguments of its ops.*_blk namesake.  A float32 bucket goes to that ops
function unchanged; a bfloat16 / float16 bucket is read as it is by the 16-bit entry points, whose
results are bit for bit the float32 ones on the widened (.float()) bucket -- without the widening
pass and its twice as large temporary.  One dtype per call; `base` stays float32; no CPU fallback.

    kblk = blk.block_scales(grads, V, bits=16, degree=world)        # then MIN across ranks
    s16, ovf, _ = blk.quantize_reduce_i16(grads, V, kblk=kblk)
    g = blk.dequantize(total, kblk, V, dtype=torch.bfloat16)
"""
from __future__ import annotations

import torch

from . import _lib, ops
from ._lib import NUM_REGISTER, check, load
from .ops import _X16, _blk_degree, _blk_scales_arg, _blk_v, _fits, _grad_bufs, _req, _req_grad, _stream


def _is16(t) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype in _X16


def _any16(bufs) -> bool:
    if isinstance(bufs, torch.Tensor):
        return _is16(bufs)
    return any(_is16(b) for b in bufs)


def _base16(base, n: int, ref: torch.Tensor, what: str):
    """The fp32 base of a 16-bit call: its device pointer or None."""
    ops._base_arg(base, n, ref, what)
    return ops._ptr(base)


def block_scales(xs, V: int, bits: int = 32, degree: int | None = None, base: torch.Tensor | None = None,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.block_scales for float32, bfloat16 or float16 buckets."""
    if not _any16(xs):
        return ops.block_scales(xs, V, bits, degree, base, out)
    V = _blk_v(V)
    if degree is not None:
        _blk_degree(degree, 0, bits)
    xs, n, xt = _grad_bufs(xs, "xs")
    degree = _blk_degree(degree, len(xs), bits)
    bp = _base16(base, n, xs[0], "xs")
    out = _blk_scales_arg(out, (n + V - 1) // V, xs[0], "out")
    check(load().ina_block_scales_x16(ops._ptrs(xs), xt, len(xs), bp, n, V, degree, bits, out.data_ptr(),
                                      _stream(xs[0])), "block_scales")
    return out


def quantize(x: torch.Tensor, kblk: torch.Tensor, V: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.quantize_blk for a float32, bfloat16 or float16 bucket."""
    if not _is16(x):
        return ops.quantize_blk(x, kblk, V, out)
    V = _blk_v(V)
    xt = _req_grad(x, "x")
    kblk = _blk_scales_arg(kblk, (x.numel() + V - 1) // V, x, given=True)
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device) if out is None else out
    _fits(out, x.numel())
    _req(out, torch.int32, "out")
    check(load().ina_quantize_blk_x16_i32(x.data_ptr(), xt, kblk.data_ptr(), V, out.data_ptr(), x.numel(),
                                          _stream(x)), "quantize_blk")
    return out


def quantize_i16(x: torch.Tensor, kblk: torch.Tensor, V: int, out=None, overflow=None):
    """ops.quantize_i16_blk for a float32, bfloat16 or float16 bucket."""
    if not _is16(x):
        return ops.quantize_i16_blk(x, kblk, V, out, overflow)
    V = _blk_v(V)
    xt = _req_grad(x, "x")
    nblk = (x.numel() + V - 1) // V
    kblk = _blk_scales_arg(kblk, nblk, x, given=True)
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device) if out is None else out
    _fits(out, x.numel())
    overflow = torch.empty(nblk, dtype=torch.uint8, device=x.device) if overflow is None else overflow
    _fits(overflow, nblk, "overflow")
    _req(out, torch.int16, "out")
    _req(overflow, torch.uint8, "overflow")
    check(load().ina_quantize_blk_x16_i16_sat(x.data_ptr(), xt, kblk.data_ptr(), V, out.data_ptr(), x.numel(),
                                              overflow.data_ptr(), _stream(x)), "quantize_i16_blk")
    return out, overflow


def quantize_reduce(bufs, V: int, kblk: torch.Tensor | None = None, degree: int | None = None,
                    out: torch.Tensor | None = None, kblk_out: torch.Tensor | None = None):
    """ops.quantize_reduce_blk for float32, bfloat16 or float16 buckets: (out, kblk)."""
    if not _any16(bufs):
        return ops.quantize_reduce_blk(bufs, V, kblk, degree, out, kblk_out)
    V = _blk_v(V)
    bufs, n, xt = _grad_bufs(bufs)
    nblk = (n + V - 1) // V
    mode = _lib.BLK_AUTO if kblk is None else _lib.BLK_GIVEN
    degree = _blk_degree(degree, len(bufs), 32) if kblk is None else 1
    kblk = _blk_scales_arg(kblk if kblk is not None else kblk_out, nblk, bufs[0])
    out = torch.empty(n, dtype=torch.int32, device=bufs[0].device) if out is None else out
    _fits(out, n)
    _req(out, torch.int32, "out")
    check(load().ina_quantize_reduce_blk_x16_i32(ops._ptrs(bufs), xt, len(bufs), kblk.data_ptr(), mode, degree, V,
                                                 out.data_ptr(), n, _stream(out)), "quantize_reduce_blk")
    return out, kblk


def quantize_reduce_i16(bufs, V: int, kblk: torch.Tensor | None = None, degree: int | None = None,
                        out=None, overflow=None, kblk_out: torch.Tensor | None = None):
    """ops.quantize_reduce_i16_blk for float32, bfloat16 or float16 buckets: (out, overflow, kblk).
    out may be bufs[0] viewed as int16 when the buckets are 16-bit."""
    if not _any16(bufs):
        return ops.quantize_reduce_i16_blk(bufs, V, kblk, degree, out, overflow, kblk_out)
    V = _blk_v(V)
    bufs, n, xt = _grad_bufs(bufs)
    nblk, dev = (n + V - 1) // V, bufs[0].device
    mode = _lib.BLK_AUTO if kblk is None else _lib.BLK_GIVEN
    degree = _blk_degree(degree, len(bufs), 16) if kblk is None else 1
    kblk = _blk_scales_arg(kblk if kblk is not None else kblk_out, nblk, bufs[0])
    out = torch.empty(n, dtype=torch.int16, device=dev) if out is None else out
    _fits(out, n)
    overflow = torch.empty(nblk, dtype=torch.uint8, device=dev) if overflow is None else overflow
    _req(out, torch.int16, "out")
    _req(overflow, torch.uint8, "overflow")
    _fits(overflow, nblk, "overflow")
    check(load().ina_quantize_reduce_blk_x16_i16_sat(ops._ptrs(bufs), xt, len(bufs), kblk.data_ptr(), mode, degree,
                                                     V, out.data_ptr(), n, overflow.data_ptr(), _stream(out)),
          "quantize_reduce_i16_blk")
    return out, overflow, kblk


def dequantize(s: torch.Tensor, kblk: torch.Tensor, V: int, out: torch.Tensor | None = None,
               dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """y = float(s) * 2^-kblk[block] as float32 (ops.dequantize_blk), or rounded once to nearest even
    to bfloat16 / float16: the dtype of `out` decides, `dtype` only when out is None."""
    if out is None and dtype != torch.float32 and dtype not in _X16:
        raise TypeError(f"dtype must be float32, bfloat16 or float16, got {dtype}")
    if not (_is16(out) or (out is None and dtype in _X16)):
        return ops.dequantize_blk(s, kblk, V, out)
    V = _blk_v(V)
    if not isinstance(s, torch.Tensor) or s.dtype not in (torch.int32, torch.int16):
        raise TypeError("s must be an int32 or int16 tensor")
    _req(s, s.dtype, "s")
    kblk = _blk_scales_arg(kblk, (s.numel() + V - 1) // V, s, given=True)
    out = torch.empty(s.shape, dtype=dtype, device=s.device) if out is None else out
    _fits(out, s.numel())
    yt = _req_grad(out, "out")
    fn = load().ina_dequantize_blk_i16_x16 if s.dtype == torch.int16 else load().ina_dequantize_blk_i32_x16
    check(fn(s.data_ptr(), kblk.data_ptr(), V, out.data_ptr(), yt, s.numel(), _stream(s)), "dequantize_blk")
    return out


def quantize_pack_nga_multi_split(xs, V: int, bitmaps, count: int, switch_id: int, seq0,
                                  base: torch.Tensor | None = None, kblk: torch.Tensor | None = None,
                                  degree: int | None = None, kblk_out: torch.Tensor | None = None,
                                  flags: int = 0, num_slots: int = NUM_REGISTER, hdrs=None, pays=None,
                                  descs=None):
    """ops.quantize_pack_nga_multi_split_blk for float32, bfloat16 or float16 buckets: (hdrs, pays,
    kblk) or (hdrs, pays, descs, kblk)."""
    if not _any16(xs):
        return ops.quantize_pack_nga_multi_split_blk(xs, V, bitmaps, count, switch_id, seq0, base, kblk, degree,
                                                     kblk_out, flags, num_slots, hdrs, pays, descs)
    V = _blk_v(V)
    xs, n, xt = _grad_bufs(xs, "xs")
    W, dev = len(xs), xs[0].device
    bp = _base16(base, n, xs[0], "xs")
    keys = ops._worker_keys(W, bitmaps, seq0)
    npk = (n + V - 1) // V
    mode = _lib.BLK_AUTO if kblk is None else _lib.BLK_GIVEN
    degree = _blk_degree(degree, W, 32) if kblk is None else 1
    kblk = _blk_scales_arg(kblk if kblk is not None else kblk_out, npk, xs[0])
    hdrs, pays = ops._worker_rows(hdrs, pays, W, npk, V, dev)
    ops._same_device(xs[0], *hdrs, *pays)
    ds = ops._worker_descs(descs, W, npk, dev)
    prm = ops._worker_params(V, keys, count, switch_id, flags, num_slots)
    check(load().ina_quantize_pack_nga_multi_split_blk_x16(ops._ptrs(xs), xt, W, bp, n, kblk.data_ptr(), mode, degree,
                                                           prm, ops._ptrs(hdrs), ops._ptrs(pays), ops._ptrs(ds),
                                                           _stream(xs[0])),
          "quantize_pack_nga_multi_split_blk")
    return (hdrs, pays, ds, kblk) if ds is not None else (hdrs, pays, kblk)
