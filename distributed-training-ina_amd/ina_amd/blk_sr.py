"""Stochastic rounding with per-block scales (include/ina_blk_sr.h): ina_amd.blk's quantisers and fused
reduces with ina_amd.sr's rounding, for float32, bfloat16 or float16 buckets.

Per element e of worker w's bucket, in block s = e // V:

    t = bufs[w][e] * 2^kblk[s];   y = floor(t) + (u < t - floor(t));   q = the sibling's clamp of y

u is 24 bits of Philox4x32-10 under the key `seed` at the counter ((e0 + e) >> 2, step, sub + w), word
(e0 + e) & 3: the random stream is ina_amd.sr's and the scale has no part in it, so on one block the
result is sr.quantize / sr.quantize_reduce on that block alone with k = kblk[s] (tests/_blk_sr_ref.py
replays it).  Computed scales follow sr.scale_for -- a whole quantum of headroom per summand -- and
the decode is ina_amd.blk's / ina_amd.wire's, which do no rounding.

    kblk = blk_sr.block_scales([grad], V, bits=16, degree=world)           # then MIN across ranks
    w = blk_sr.quantize_i16_wire(grad_bf16, kblk, V, seed, step=t, sub=rank)
    s16, ovf, kblk = blk_sr.quantize_reduce_i16(slices, V, seed, degree=W, step=t, e0=lo)   # AUTO scales

One dtype per call; no base (the round-to-nearest siblings take none in the quantisers); no CPU
fallback.  There is no standalone int16 quantiser: quantize_reduce_i16 of one bucket with given scales
is that operation.  dist.BlockStochasticAggregator and dist.BlockStochasticRangeAggregator are the two
layouts of config 5 on these calls.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops, sr
from ._lib import check, load
from .ops import _blk_scales_arg, _blk_v, _fits, _grad_bufs, _ptr, _ptrs, _req, _req_grad, _same_device, _stream
from .sr import _blk_degree, _params


def block_scales(xs, V: int, bits: int = 32, degree: int | None = None, base: torch.Tensor | None = None,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """blk.block_scales under sr.scale_for's rule, for float32, bfloat16 or float16 buckets: for each block
    of V values the k that ina_scale_for_sr gives for the block's max |xs[w][i] - base[i]|, `degree`
    summands (default: the number of buckets) and `bits`.  Ranks agree on a block's scale by taking the
    MIN of theirs."""
    V = _blk_v(V)
    if degree is not None:
        _blk_degree(degree, 0, bits)
    xs, n, xt = _grad_bufs(xs, "xs")
    degree = _blk_degree(degree, len(xs), bits)
    ops._base_arg(base, n, xs[0], "xs")
    out = _blk_scales_arg(out, (n + V - 1) // V, xs[0], "out")
    if xt:
        rc = load().ina_block_scales_sr_x16(_ptrs(xs), xt, len(xs), _ptr(base), n, V, degree, bits, out.data_ptr(),
                                            _stream(xs[0]))
    else:
        rc = load().ina_block_scales_sr_f32(_ptrs(xs), len(xs), _ptr(base), n, V, degree, bits, out.data_ptr(),
                                            _stream(xs[0]))
    check(rc, "blk_sr.block_scales")
    return out


def _one(x: torch.Tensor, kblk, V: int, out):
    """A single bucket with given scales and its int32 out: (V, type code, kblk, out)."""
    V = _blk_v(V)
    xt = _req_grad(x, "x")
    kblk = _blk_scales_arg(kblk, (x.numel() + V - 1) // V, x, given=True)
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device) if out is None else out
    _fits(out, x.numel())
    _req(out, torch.int32, "out")
    _same_device(x, out)
    return V, xt, kblk, out


def quantize(x: torch.Tensor, kblk: torch.Tensor, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0,
             out: torch.Tensor | None = None) -> torch.Tensor:
    """blk.quantize rounded stochastically: int32, block s scaled by 2^kblk[s]."""
    prm = _params(seed, step, sub, e0)
    V, xt, kblk, out = _one(x, kblk, V, out)
    if xt:
        rc = load().ina_quantize_blk_sr_x16_i32(x.data_ptr(), xt, kblk.data_ptr(), V, out.data_ptr(), x.numel(),
                                                C.byref(prm), _stream(x))
    else:
        rc = load().ina_quantize_blk_sr_f32_i32(x.data_ptr(), kblk.data_ptr(), V, out.data_ptr(), x.numel(),
                                                C.byref(prm), _stream(x))
    check(rc, "blk_sr.quantize")
    return out


def quantize_i16_wire(x: torch.Tensor, kblk: torch.Tensor, V: int, seed: int, step: int = 0, sub: int = 0,
                      e0: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """wire.quantize_blk rounded stochastically: the int32 wire words q16 + (saturated << 22) of
    dist.BlockStochasticAggregator(wire="i16")."""
    prm = _params(seed, step, sub, e0)
    V, xt, kblk, out = _one(x, kblk, V, out)
    if xt:
        rc = load().ina_quantize_blk_sr_x16_i16_wire(x.data_ptr(), xt, kblk.data_ptr(), V, out.data_ptr(), x.numel(),
                                                     C.byref(prm), _stream(x))
    else:
        rc = load().ina_quantize_blk_sr_f32_i16_wire(x.data_ptr(), kblk.data_ptr(), V, out.data_ptr(), x.numel(),
                                                     C.byref(prm), _stream(x))
    check(rc, "blk_sr.quantize_i16_wire")
    return out


def _reduce_args(bufs, V, seed, kblk, degree, step, sub, e0, out, kblk_out, bits):
    prm = _params(seed, step, sub, e0)
    V = _blk_v(V)
    bufs, n, xt = _grad_bufs(bufs)
    nblk = (n + V - 1) // V
    mode = _lib.BLK_AUTO if kblk is None else _lib.BLK_GIVEN
    degree = _blk_degree(degree, len(bufs), bits) if kblk is None else 1
    kblk = _blk_scales_arg(kblk if kblk is not None else kblk_out, nblk, bufs[0])
    dt = torch.int32 if bits == 32 else torch.int16
    out = torch.empty(n, dtype=dt, device=bufs[0].device) if out is None else out
    _fits(out, n)
    _req(out, dt, "out")
    _same_device(bufs[0], out)
    return prm, V, bufs, n, xt, nblk, mode, degree, kblk, out


def quantize_reduce(bufs, V: int, seed: int, kblk: torch.Tensor | None = None, degree: int | None = None,
                    step: int = 0, sub: int = 0, e0: int = 0, out: torch.Tensor | None = None,
                    kblk_out: torch.Tensor | None = None):
    """blk.quantize_reduce with every summand rounded stochastically, one launch: (out, kblk) -- the int32
    sum (mod 2^32) over w of blk_sr.quantize(bufs[w], kblk, V, seed, step, sub + w, e0).  kblk=None
    computes the scales in the same launch for `degree` summands (default: the number of buckets) under
    sr.scale_for's rule and returns them (in kblk_out when given); a given kblk is read."""
    prm, V, bufs, n, xt, _, mode, degree, kblk, out = _reduce_args(bufs, V, seed, kblk, degree, step, sub, e0, out,
                                                                   kblk_out, 32)
    if xt:
        rc = load().ina_quantize_reduce_blk_sr_x16_i32(_ptrs(bufs), xt, len(bufs), kblk.data_ptr(), mode, degree, V,
                                                       out.data_ptr(), n, C.byref(prm), _stream(out))
    else:
        rc = load().ina_quantize_reduce_blk_sr_f32_i32(_ptrs(bufs), len(bufs), kblk.data_ptr(), mode, degree, V,
                                                       out.data_ptr(), n, C.byref(prm), _stream(out))
    check(rc, "blk_sr.quantize_reduce")
    return out, kblk


def quantize_reduce_i16(bufs, V: int, seed: int, kblk: torch.Tensor | None = None, degree: int | None = None,
                        step: int = 0, sub: int = 0, e0: int = 0, out=None, overflow=None,
                        kblk_out: torch.Tensor | None = None):
    """blk.quantize_reduce_i16 with every summand rounded stochastically, one launch: (out int16, overflow,
    kblk) -- each summand saturated at int16, the sum saturated once, one flag per block (1 where a
    summand or the sum saturated or a value was NaN).  One bucket with given scales is the int16
    quantiser.  With e0 != 0 the caller keeps e0 a multiple of V."""
    prm, V, bufs, n, xt, nblk, mode, degree, kblk, out = _reduce_args(bufs, V, seed, kblk, degree, step, sub, e0,
                                                                      out, kblk_out, 16)
    overflow = torch.empty(nblk, dtype=torch.uint8, device=out.device) if overflow is None else overflow
    _fits(overflow, nblk, "overflow")
    _req(overflow, torch.uint8, "overflow")
    _same_device(out, overflow)
    if xt:
        rc = load().ina_quantize_reduce_blk_sr_x16_i16_sat(_ptrs(bufs), xt, len(bufs), kblk.data_ptr(), mode, degree,
                                                           V, out.data_ptr(), n, overflow.data_ptr(), C.byref(prm),
                                                           _stream(out))
    else:
        rc = load().ina_quantize_reduce_blk_sr_f32_i16_sat(_ptrs(bufs), len(bufs), kblk.data_ptr(), mode, degree, V,
                                                           out.data_ptr(), n, overflow.data_ptr(), C.byref(prm),
                                                           _stream(out))
    check(rc, "blk_sr.quantize_reduce_i16")
    return out, overflow, kblk


scale_for = sr.scale_for
