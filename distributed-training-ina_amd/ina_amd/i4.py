"""The 4-bit wire of the sharded step (include/ina_i4.h), for float32, bfloat16 or float16 buckets.

ina_amd.i8's step with half the bytes in the all-to-all: a rank quantises its bucket to signed nibbles in [-7, 7]
under per-block scales -- with `rotate=seed` after ina_amd.rot's rotation of each block of V values, which is what
makes 4 bits worth sending -- packs two to a byte (even values in the low nibble), sends slice j to rank j, and the
owner adds the G nibbles of every value as integers, exactly.  The sums decode with what is there already:

    kblk = i4.block_scales([grad], V, rotate=seed, step=t)          # then MIN across ranks
    q4, flags = i4.quantize(grad, kblk, V, rotate=seed, step=t)     # uint8 [n / 2], two values a byte
    q8s, sh = i4.sum_slices_requant(received, V)                    # int8 + one uint8 shift a block (0..3)
    g = i8.dequantize_gather(gathered, shifts, kblk, V, rotate=seed, step=t)

or, with the int16 sums on the gather,

    s16 = i4.sum_slices(received)                                   # int16, exact
    g = rot.dequantize(gathered, kblk, V, seed, step=t)

Up to 18 ranks the sums fit a byte (7 * 18 = 126): every shift is 0 and the requantising sum loses nothing.
dist.NibbleWireAggregator runs the step; tests/_i4_ref.py replays the contract.

`rotate` is None (no rotation) or the seed.  n must be a multiple of V for the block calls and of 8 for the exact
sum, buffers 16-byte aligned, e0 a multiple of 128 and of V; no CPU fallback and no value-by-value path.
"""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import MAX_WORKERS, check, load
from .i8 import _sr
from .ops import _blk_scales_arg, _fits, _grad_bufs, _ptrs, _req, _req_grad, _same_device, _stream
from .rot import _v


def scale_for(absmax: float) -> int:
    """The largest k in [-126, 127] with absmax * 2^k + 1/2 <= 7, whatever the number of ranks."""
    k = C.c_int(0)
    check(load().ina_scale_for_i4(float(absmax), C.byref(k)), "i4.scale_for")
    return k.value


def block_scales(xs, V: int, rotate: int | None = None, step: int = 0, sub: int = 0, e0: int = 0,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """int8 [n / V]: for each block scale_for(max |r|) over the given buckets, r the rotated values under
    `rotate`.  Ranks of one job agree on a block's scale by taking the MIN of theirs."""
    xs, n, xt = _grad_bufs(xs, "xs")
    V = _v(V, n)
    prm = _sr(rotate, step, sub, e0, V)
    out = _blk_scales_arg(out, n // V, xs[0], "out")
    check(load().ina_block_scales_i4(_ptrs(xs), xt, len(xs), n, V, out.data_ptr(), prm, _stream(xs[0])),
          "i4.block_scales")
    return out


def quantize(x: torch.Tensor, kblk: torch.Tensor, V: int, rotate: int | None = None, step: int = 0, sub: int = 0,
             e0: int = 0, out: torch.Tensor | None = None, overflow: torch.Tensor | None = None):
    """(uint8 [n / 2], flags): the nibbles clamp(rne(r * 2^kblk[block]), -7, 7), NaN -> 0, value e in byte e / 2
    (even e low); one rank-local flag per block, 1 where a value clamped or was NaN."""
    xt = _req_grad(x, "x")
    n = x.numel()
    V = _v(V, n)
    prm = _sr(rotate, step, sub, e0, V)
    kblk = _blk_scales_arg(kblk, n // V, x, given=True)
    out = torch.empty(n // 2, dtype=torch.uint8, device=x.device) if out is None else out
    _fits(out, n // 2)
    _req(out, torch.uint8, "out")
    overflow = torch.empty(n // V, dtype=torch.uint8, device=x.device) if overflow is None else overflow
    _fits(overflow, n // V, "overflow")
    _req(overflow, torch.uint8, "overflow")
    _same_device(x, out, overflow)
    check(load().ina_quantize_i4_wire(x.data_ptr(), xt, kblk.data_ptr(), V, out.data_ptr(), n, overflow.data_ptr(),
                                      prm, _stream(x)), "i4.quantize")
    return out, overflow


def _nibble_slices(parts, n):
    """The 1..64 uint8 slices of a sum, of one length, and the number of values n (two a byte)."""
    parts = list(parts.unbind(0)) if isinstance(parts, torch.Tensor) and parts.dim() > 1 else list(parts)
    if not 1 <= len(parts) <= MAX_WORKERS:
        raise ValueError(f"1..{MAX_WORKERS} slices, got {len(parts)}")
    for p in parts:
        _req(p, torch.uint8, "parts")
    nbytes = parts[0].numel()
    if any(p.numel() != nbytes for p in parts):
        raise ValueError("every slice must hold the same number of bytes")
    n = 2 * nbytes if n is None else int(n)
    if n < 0 or n > 2 * nbytes:
        raise ValueError(f"the slices hold {2 * nbytes} values, n is {n}")
    return parts, n


def sum_slices(parts, n: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """int16 [n]: the exact element-wise sum of 1..64 slices of packed nibbles, n values each (a multiple of 8;
    by default all that the slices hold), -8 included."""
    parts, n = _nibble_slices(parts, n)
    if n % 8:
        raise ValueError(f"n must be a multiple of 8, got {n}")
    out = torch.empty(n, dtype=torch.int16, device=parts[0].device) if out is None else out
    _fits(out, n)
    _req(out, torch.int16, "out")
    _same_device(out, *parts)
    check(load().ina_sum_i4_slices(_ptrs(parts), len(parts), out.data_ptr(), n, _stream(out)), "i4.sum_slices")
    return out


def sum_slices_requant(parts, V: int, out: torch.Tensor | None = None, shift: torch.Tensor | None = None):
    """(int8 [n], uint8 [n / V]): the exact sum of 1..64 slices of packed nibbles, each block of V sums rounded to
    nearest even under the block's shift, i8.sum_slices_requant's rule -- here 0 up to 18 slices and at most 3.
    i8.dequantize_gather decodes the result."""
    parts, n = _nibble_slices(parts, None)
    V = _v(V, n)
    out = torch.empty(n, dtype=torch.int8, device=parts[0].device) if out is None else out
    _fits(out, n)
    _req(out, torch.int8, "out")
    shift = torch.empty(n // V, dtype=torch.uint8, device=out.device) if shift is None else shift
    _fits(shift, n // V, "shift")
    _req(shift, torch.uint8, "shift")
    _same_device(out, shift, *parts)
    check(load().ina_sum_i4_slices_requant(_ptrs(parts), len(parts), V, out.data_ptr(), shift.data_ptr(), n,
                                           _stream(out)), "i4.sum_slices_requant")
    return out, shift
