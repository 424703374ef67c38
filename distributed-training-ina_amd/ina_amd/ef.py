"""Error feedback for the quantiser (include/ina_ef.h): the worker keeps what rounding dropped.

A worker owns one float32 residual per bucket.  It starts at zero (new_residual) and every call
here adds it to the gradient, quantises the sum and writes the new residual back in place, in the
quantiser's own launch:

    v = (x - base) + r;   q = Q(v, k);   r' = v - float(q) * 2^-k   (+0 where v is NaN or inf)

so the sum of what was sent tracks the sum of what was meant to be sent.  Q, its saturation and
its flags are those of the ops function of the same name; with a zero residual every result equals
that function's bit for bit.  The switch and the PS see plain integers, as before.

    r = ef.new_residual(grad)
    for step in ...:
        q = ef.quantize(grad, r, k)                       # r updated in place
        kblk = ef.block_scales([grad], [r], V)            # then MIN across ranks
        q, kblk = ef.quantize_blk(grad, r, V, kblk=kblk)
        wire = ef.quantize_i16_wire(grad, r, k)           # the sharded int16 wire's words

x is float32, bfloat16 or float16 on the global-k quantisers and float32 everywhere else; resid and
base are float32.  No CPU fallback.
"""
from __future__ import annotations

import numbers

import torch

from . import _lib, ops
from ._lib import NUM_REGISTER, check, load
from .ops import _X16, _blk_degree, _blk_scales_arg, _blk_v, _fits, _ptr, _ptrs, _req, _req_grad, _same_device, _stream


def new_residual(x: torch.Tensor) -> torch.Tensor:
    """The zero residual of bucket x: float32, x's shape and device, whatever x's dtype."""
    _req_grad(x, "x")
    return torch.zeros(x.shape, dtype=torch.float32, device=x.device)


def _f32(t, name: str):
    """The block-scaled and pack calls take fp32 buckets: a bf16 / fp16 tensor is refused as such."""
    if isinstance(t, torch.Tensor) and t.dtype in _X16:
        raise ValueError(f"error feedback with block scales or packs takes fp32 buckets: {name} is {t.dtype}")
    _req(t, torch.float32, name)


def _resid(resid, ref: torch.Tensor, name: str = "resid"):
    _req(resid, torch.float32, name)
    if resid.numel() != ref.numel():
        raise ValueError(f"{name} holds {resid.numel()} elements, the bucket {ref.numel()}")
    _same_device(ref, resid)


def _bufs(xs, resids):
    """W fp32 buckets and their W residuals: (xs, resids, n)."""
    xs = [xs] if isinstance(xs, torch.Tensor) else list(xs)
    resids = [resids] if isinstance(resids, torch.Tensor) else list(resids)
    if not 1 <= len(xs) <= _lib.MAX_WORKERS:
        raise ValueError(f"W must be in [1, {_lib.MAX_WORKERS}]")
    if len(resids) != len(xs):
        raise ValueError("one residual per bucket")
    for i, (x, r) in enumerate(zip(xs, resids)):
        _f32(x, f"xs[{i}]")
        if x.numel() != xs[0].numel():
            raise ValueError("all buckets must have the same length")
        _same_device(xs[0], x)
        _resid(r, x, f"resids[{i}]")
    return xs, resids, xs[0].numel()


def quantize(x: torch.Tensor, resid: torch.Tensor, k: int, base: torch.Tensor | None = None,
             out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.quantize of (x - base) + resid; resid becomes what rounding dropped."""
    xt = _req_grad(x, "x")
    _resid(resid, x)
    ops._base_arg(base, x.numel(), x, "x")
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device) if out is None else out
    _fits(out, x.numel())
    _req(out, torch.int32, "out")
    if xt:
        rc = load().ina_quantize_ef_x16_i32(x.data_ptr(), xt, _ptr(base), resid.data_ptr(), out.data_ptr(), x.numel(),
                                            k, _stream(x))
    else:
        rc = load().ina_quantize_ef_f32_i32(x.data_ptr(), _ptr(base), resid.data_ptr(), out.data_ptr(), x.numel(), k,
                                            _stream(x))
    check(rc, "ef.quantize")
    return out


def quantize_i16(x: torch.Tensor, resid: torch.Tensor, k: int, V: int, base: torch.Tensor | None = None,
                 out=None, overflow=None):
    """ops.quantize_i16 of (x - base) + resid: (out, overflow).  A value that saturates carries the
    clipped part forward in resid."""
    xt = _req_grad(x, "x")
    _resid(resid, x)
    ops._base_arg(base, x.numel(), x, "x")
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device) if out is None else out
    _fits(out, x.numel())
    nslot = (x.numel() + V - 1) // V
    overflow = torch.empty(nslot, dtype=torch.uint8, device=x.device) if overflow is None else overflow
    _fits(overflow, nslot, "overflow")
    _req(out, torch.int16, "out")
    _req(overflow, torch.uint8, "overflow")
    if xt:
        rc = load().ina_quantize_ef_x16_i16_sat(x.data_ptr(), xt, _ptr(base), resid.data_ptr(), out.data_ptr(),
                                                x.numel(), k, V, overflow.data_ptr(), _stream(x))
    else:
        rc = load().ina_quantize_ef_f32_i16_sat(x.data_ptr(), _ptr(base), resid.data_ptr(), out.data_ptr(), x.numel(),
                                                k, V, overflow.data_ptr(), _stream(x))
    check(rc, "ef.quantize_i16")
    return out, overflow


def block_scales(xs, resids, V: int, bits: int = 32, degree: int | None = None,
                 base: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.block_scales over |(xs[w] - base) + resids[w]|: what the next block-scaled EF call will
    quantise.  Nothing but the scales is written; ranks agree by taking the MIN of theirs."""
    V = _blk_v(V)
    if degree is not None:
        _blk_degree(degree, 0, bits)
    xs, resids, n = _bufs(xs, resids)
    degree = _blk_degree(degree, len(xs), bits)
    ops._base_arg(base, n, xs[0], "xs")
    out = _blk_scales_arg(out, (n + V - 1) // V, xs[0], "out")
    check(load().ina_block_scales_ef_f32(_ptrs(xs), _ptrs(resids), len(xs), _ptr(base), n, V, degree, bits,
                                         out.data_ptr(), _stream(xs[0])), "ef.block_scales")
    return out


def _blk_call(x, resid, V, kblk, degree, base, kblk_out, bits):
    V = _blk_v(V)
    _f32(x, "x")
    _resid(resid, x)
    ops._base_arg(base, x.numel(), x, "x")
    nblk = (x.numel() + V - 1) // V
    mode = _lib.BLK_AUTO if kblk is None else _lib.BLK_GIVEN
    degree = _blk_degree(degree, 1, bits) if kblk is None else 1
    kblk = _blk_scales_arg(kblk if kblk is not None else kblk_out, nblk, x)
    return V, nblk, mode, degree, kblk


def quantize_blk(x: torch.Tensor, resid: torch.Tensor, V: int, kblk: torch.Tensor | None = None,
                 degree: int | None = None, base: torch.Tensor | None = None, out: torch.Tensor | None = None,
                 kblk_out: torch.Tensor | None = None):
    """ops.quantize_blk of (x - base) + resid: (out, kblk).  kblk=None computes the scales in the
    same launch for `degree` summands (default 1) and returns them (in kblk_out when given)."""
    V, nblk, mode, degree, kblk = _blk_call(x, resid, V, kblk, degree, base, kblk_out, 32)
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device) if out is None else out
    _fits(out, x.numel())
    _req(out, torch.int32, "out")
    check(load().ina_quantize_ef_blk_f32_i32(x.data_ptr(), _ptr(base), resid.data_ptr(), kblk.data_ptr(), mode, degree,
                                             V, out.data_ptr(), x.numel(), _stream(x)), "ef.quantize_blk")
    return out, kblk


def quantize_i16_blk(x: torch.Tensor, resid: torch.Tensor, V: int, kblk: torch.Tensor | None = None,
                     degree: int | None = None, base: torch.Tensor | None = None, out=None, overflow=None,
                     kblk_out: torch.Tensor | None = None):
    """ops.quantize_i16_blk of (x - base) + resid: (out, overflow, kblk); kblk=None as in quantize_blk,
    at 16 bits."""
    V, nblk, mode, degree, kblk = _blk_call(x, resid, V, kblk, degree, base, kblk_out, 16)
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device) if out is None else out
    _fits(out, x.numel())
    overflow = torch.empty(nblk, dtype=torch.uint8, device=x.device) if overflow is None else overflow
    _fits(overflow, nblk, "overflow")
    _req(out, torch.int16, "out")
    _req(overflow, torch.uint8, "overflow")
    check(load().ina_quantize_ef_blk_f32_i16_sat(x.data_ptr(), _ptr(base), resid.data_ptr(), kblk.data_ptr(), mode,
                                                 degree, V, out.data_ptr(), x.numel(), overflow.data_ptr(),
                                                 _stream(x)), "ef.quantize_i16_blk")
    return out, overflow, kblk


def _wire_x(x):
    """The sharded int16 wire has no 16-bit source path: a bf16 / fp16 tensor is refused as such."""
    if isinstance(x, torch.Tensor) and x.dtype in _X16:
        raise ValueError(f"the sharded int16 wire takes fp32 buckets: x is {x.dtype}")
    _req(x, torch.float32, "x")


def _wire_out(x: torch.Tensor, out):
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device) if out is None else out
    _fits(out, x.numel())
    _req(out, torch.int32, "out")
    _same_device(x, out)
    return out


def quantize_i16_wire(x: torch.Tensor, resid: torch.Tensor, k: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.quantize_i16_wire of x + resid (include/ina_shard_ef.h): the int32 wire words q16 +
    (saturated << 22) of dist.ShardedAggregator(wire="i16", error_feedback=True).  resid becomes
    v - float(q16) * 2^-k: the word's q16, never its count bits.  fp32 only."""
    _wire_x(x)
    _resid(resid, x)
    out = _wire_out(x, out)
    check(load().ina_quantize_ef_f32_i16_wire(x.data_ptr(), resid.data_ptr(), out.data_ptr(), x.numel(), k,
                                              _stream(x)), "ef.quantize_i16_wire")
    return out


def quantize_i16_wire_blk(x: torch.Tensor, resid: torch.Tensor, kblk: torch.Tensor, V: int,
                          out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.quantize_i16_wire_blk of x + resid with the given scales (the ranks agree on them first:
    the MIN of their ef.block_scales([x], [resid], V, bits=16, degree=world))."""
    V = _blk_v(V)
    _wire_x(x)
    _resid(resid, x)
    kblk = _blk_scales_arg(kblk, (x.numel() + V - 1) // V, x, given=True)
    out = _wire_out(x, out)
    check(load().ina_quantize_ef_blk_f32_i16_wire(x.data_ptr(), resid.data_ptr(), kblk.data_ptr(), V, out.data_ptr(),
                                                  x.numel(), _stream(x)), "ef.quantize_i16_wire_blk")
    return out


def quantize_pack_nga_multi_split(xs, resids, k, V: int, bitmaps, count: int, switch_id: int, seq0,
                                  base: torch.Tensor | None = None, degree: int | None = None,
                                  kblk_out: torch.Tensor | None = None, flags: int = 0,
                                  num_slots: int = NUM_REGISTER, hdrs=None, pays=None, descs=None):
    """W workers' error-feedback quantise + split pack in one launch.  k an int:
    ops.quantize_pack_nga_multi_split, returns (hdrs, pays) or (hdrs, pays, descs).  k an int8
    tensor (one scale per packet) or None (the scales computed from these workers' v for `degree`
    summands): ops.quantize_pack_nga_multi_split_blk, returns the same plus the scales.  Each
    resids[w] is updated in place."""
    if k is not None and not isinstance(k, (numbers.Integral, torch.Tensor)):
        raise TypeError("k must be an int, an int8 tensor of per-packet scales, or None")
    blk = not isinstance(k, numbers.Integral)
    if blk:
        V = _blk_v(V)
    xs, resids, n = _bufs(xs, resids)
    W, dev = len(xs), xs[0].device
    ops._base_arg(base, n, xs[0], "xs")
    keys = ops._worker_keys(W, bitmaps, seq0)
    npk = (n + V - 1) // V
    if blk:
        mode = _lib.BLK_AUTO if k is None else _lib.BLK_GIVEN
        degree = _blk_degree(degree, W, 32) if k is None else 1
        kblk = _blk_scales_arg(k if k is not None else kblk_out, npk, xs[0])
    hdrs, pays = ops._worker_rows(hdrs, pays, W, npk, V, dev)
    _same_device(xs[0], *hdrs, *pays)
    ds = ops._worker_descs(descs, W, npk, dev)
    prm = ops._worker_params(V, keys, count, switch_id, flags, num_slots)
    xa, ra, ha, pa, da = _ptrs(xs), _ptrs(resids), _ptrs(hdrs), _ptrs(pays), _ptrs(ds)
    if blk:
        rc = load().ina_quantize_pack_nga_multi_split_ef_blk(xa, ra, W, _ptr(base), n, kblk.data_ptr(), mode, degree,
                                                             prm, ha, pa, da, _stream(xs[0]))
    else:
        rc = load().ina_quantize_pack_nga_multi_split_ef(xa, ra, W, _ptr(base), n, int(k), prm, ha, pa, da,
                                                         _stream(xs[0]))
    check(rc, "ef.quantize_pack_nga_multi_split")
    res = (hdrs, pays, ds) if ds is not None else (hdrs, pays)
    return res + (kblk,) if blk else res
