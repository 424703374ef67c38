"""A randomised Hadamard rotation in front of the block-scaled quantise and reduce (include/ina_rot.h), for
float32, bfloat16 or float16 buckets.

Inside one block the quantum is set by the block's largest value.  Each block of V values (a power of two in
[8, 256]) is multiplied by a diagonal of shared random signs and Walsh-Hadamard transformed before
ina_amd.blk's quantiser runs on it: the rotated block's largest value is a few times its RMS instead of up to
sqrt(V) times, so the quantum shrinks by that ratio.  The rotation is linear and the same on every worker and
rank (the signs come from Philox4x32-10 under `seed` at (step, sub), element e0 + e -- never sub + w), so
integers still add on the wire; dequantize() undoes it once.  tests/_rot_ref.py replays the contract.

    kblk = rot.block_scales([grad], V, seed, bits=16, degree=world, step=t)     # then MIN across ranks
    s16, ovf, kblk = rot.quantize_reduce_i16(grads, V, seed, step=t)            # AUTO scales
    g = rot.dequantize(total, kblk, V, seed, step=t)

n must be a multiple of V, buffers 16-byte aligned, e0 a multiple of 128 and of V; one dtype per call; no
base; no CPU fallback and no value-by-value path.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check, load
from .ops import (_blk_degree, _blk_scales_arg, _fits, _grad_bufs, _ptrs, _req, _same_device, _stream)
from .sr import _params


def _v(V, n: int) -> int:
    V = int(V)
    if V < 8 or V > 256 or V & (V - 1):
        raise ValueError(f"V must be a power of two in [8, 256], got {V}")
    if n % V:
        raise ValueError(f"n must be a multiple of V: {n} values in blocks of {V}")
    return V


def _key(seed, step, sub, e0, V: int) -> _lib.SrParams:
    prm = _params(seed, step, sub, e0)
    if e0 % 128 or e0 % V:
        raise ValueError(f"e0 must be a multiple of 128 and of V, got {e0}")
    return prm


def block_scales(xs, V: int, seed: int, bits: int = 32, degree: int | None = None, step: int = 0, sub: int = 0,
                 e0: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """int8 [n / V]: for each block the k that ina_scale_for gives for the max |rotated value| over the given
    buckets, `degree` summands (default: the number of buckets) and `bits`.  Ranks of one job agree on a
    block's scale by taking the MIN of theirs."""
    if degree is not None:
        _blk_degree(degree, 0, bits)
    xs, n, xt = _grad_bufs(xs, "xs")
    V = _v(V, n)
    degree = _blk_degree(degree, len(xs), bits)
    prm = _key(seed, step, sub, e0, V)
    out = _blk_scales_arg(out, n // V, xs[0], "out")
    check(load().ina_block_scales_rot(_ptrs(xs), xt, len(xs), n, V, degree, bits, out.data_ptr(), C.byref(prm),
                                      _stream(xs[0])), "rot.block_scales")
    return out


def _reduce_args(bufs, V, seed, kblk, degree, step, sub, e0, out, kblk_out, bits):
    bufs, n, xt = _grad_bufs(bufs)
    V = _v(V, n)
    prm = _key(seed, step, sub, e0, V)
    mode = _lib.BLK_AUTO if kblk is None else _lib.BLK_GIVEN
    degree = _blk_degree(degree, len(bufs), bits) if kblk is None else 1
    kblk = _blk_scales_arg(kblk if kblk is not None else kblk_out, n // V, bufs[0])
    dt = torch.int32 if bits == 32 else torch.int16
    out = torch.empty(n, dtype=dt, device=bufs[0].device) if out is None else out
    _fits(out, n)
    _req(out, dt, "out")
    _same_device(bufs[0], out)
    return prm, V, bufs, n, xt, mode, degree, kblk, out


def quantize_reduce(bufs, V: int, seed: int, kblk: torch.Tensor | None = None, degree: int | None = None,
                    step: int = 0, sub: int = 0, e0: int = 0, out: torch.Tensor | None = None,
                    kblk_out: torch.Tensor | None = None):
    """Rotate + quantise + W-way sum in one launch: (out int32, kblk).  One bucket is the plain quantiser.
    kblk=None computes the scales of the rotated values in the same launch for `degree` summands (default:
    the number of buckets) and returns them (in kblk_out when given); a given kblk is read."""
    prm, V, bufs, n, xt, mode, degree, kblk, out = _reduce_args(bufs, V, seed, kblk, degree, step, sub, e0, out,
                                                                kblk_out, 32)
    check(load().ina_quantize_reduce_rot_i32(_ptrs(bufs), xt, len(bufs), kblk.data_ptr(), mode, degree, V,
                                             out.data_ptr(), n, C.byref(prm), _stream(out)), "rot.quantize_reduce")
    return out, kblk


def quantize_reduce_i16(bufs, V: int, seed: int, kblk: torch.Tensor | None = None, degree: int | None = None,
                        step: int = 0, sub: int = 0, e0: int = 0, out=None, overflow=None,
                        kblk_out: torch.Tensor | None = None):
    """The same to int16: (out, overflow, kblk) -- each summand saturated at int16, the sum saturated once,
    one flag per block (1 where a summand or the sum saturated or a rotated value was NaN)."""
    prm, V, bufs, n, xt, mode, degree, kblk, out = _reduce_args(bufs, V, seed, kblk, degree, step, sub, e0, out,
                                                                kblk_out, 16)
    overflow = torch.empty(n // V, dtype=torch.uint8, device=out.device) if overflow is None else overflow
    _fits(overflow, n // V, "overflow")
    _req(overflow, torch.uint8, "overflow")
    _same_device(out, overflow)
    check(load().ina_quantize_reduce_rot_i16_sat(_ptrs(bufs), xt, len(bufs), kblk.data_ptr(), mode, degree, V,
                                                 out.data_ptr(), n, overflow.data_ptr(), C.byref(prm), _stream(out)),
          "rot.quantize_reduce_i16")
    return out, overflow, kblk


def dequantize(s: torch.Tensor, kblk: torch.Tensor, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """float32: float(s) * 2^-kblk[block], then the inverse rotation; s: int32 or int16."""
    if not isinstance(s, torch.Tensor) or s.dtype not in (torch.int32, torch.int16):
        raise TypeError("s must be an int32 or int16 tensor")
    _req(s, s.dtype, "s")
    V = _v(V, s.numel())
    prm = _key(seed, step, sub, e0, V)
    kblk = _blk_scales_arg(kblk, s.numel() // V, s, given=True)
    out = torch.empty(s.shape, dtype=torch.float32, device=s.device) if out is None else out
    _fits(out, s.numel())
    _req(out, torch.float32, "out")
    _same_device(s, out)
    fn = load().ina_dequantize_rot_i16 if s.dtype == torch.int16 else load().ina_dequantize_rot_i32
    check(fn(s.data_ptr(), kblk.data_ptr(), V, out.data_ptr(), s.numel(), C.byref(prm), _stream(s)), "rot.dequantize")
    return out


def ps_combine_ina(local: torch.Tensor, paras, V: int, weight_step: float, seed: int, step: int = 0, sub: int = 0,
                   e0: int = 0, out=None, kblk_out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.ps_combine_ina_blk with the rotation on both sides of the integer sum, in one launch: bit for bit
    quantize_reduce (AUTO) of the deltas paras[w] - local, dequantize, then local + xhat * float(weight_step)."""
    _req(local, torch.float32, "local")
    paras, n, xt = _grad_bufs(paras, "paras")
    if xt:
        raise TypeError("the PS combine takes float32 parameters")
    if n != local.numel():
        raise ValueError("local and paras differ in length")
    V = _v(V, n)
    prm = _key(seed, step, sub, e0, V)
    _same_device(local, paras[0])
    out = torch.empty_like(local) if out is None else out
    _fits(out, n)
    _req(out, torch.float32, "out")
    if kblk_out is not None:
        kblk_out = _blk_scales_arg(kblk_out, n // V, local, "kblk_out")
    check(load().ina_ps_combine_ina_rot_f32(local.data_ptr(), _ptrs(paras), len(paras), V, float(weight_step),
                                            out.data_ptr(), n, kblk_out.data_ptr() if kblk_out is not None else None,
                                            C.byref(prm), _stream(local)), "rot.ps_combine_ina")
    return out
