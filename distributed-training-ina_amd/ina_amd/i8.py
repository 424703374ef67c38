"""The 8-bit wire of the sharded step (include/ina_i8.h), for float32, bfloat16 or float16 buckets.

A rank quantises its bucket to bytes in [-127, 127] under per-block scales -- with `rotate=seed` after
ina_amd.rot's rotation of each block of V values, which is what makes 8 bits enough -- sends slice j to rank j
in one all-to-all, and the owner adds the G bytes of every value into an int16, exactly (64 * 128 fits).  The
sums decode with rot.dequantize (rotated) or blk.dequantize (plain) under the agreed scales.
dist.ByteWireAggregator runs the step; tests/_i8_ref.py replays the contract.

    kblk = i8.block_scales([grad], V, rotate=seed, step=t)          # then MIN across ranks
    q8 = i8.quantize(grad, kblk, V, rotate=seed, step=t)            # int8, one byte a value
    s16 = i8.sum_slices(received)                                   # int16, exact
    g = rot.dequantize(gathered, kblk, V, seed, step=t)

The gather may carry bytes instead of the int16 sums (include/ina_i8_gather.h; ByteWireAggregator(gather="i8")):
the owner rounds each block of its sums back to bytes under a per-block shift in the launch that sums them, and
the decode reads those bytes -- one byte a value more off the links, half of 2^shift summand quanta more error.

    q8s, sh = i8.sum_slices_requant(received, V)                    # int8 + one uint8 shift a block
    g = i8.dequantize_gather(gathered, shifts, kblk, V, rotate=seed, step=t)

A rank may keep what its bytes dropped (include/ina_i8_ef.h; ByteWireAggregator(error_feedback=True)): one fp32
residual per bucket, added in front of the rotation and rewritten in the quantiser's launch with the rounding
error taken back through the inverse rotation.  It never travels, and nothing else of the step changes.

    kblk = i8.block_scales_ef([grad], [resid], V, rotate=seed, step=t)      # then MIN across ranks
    q8, flags = i8.quantize_ef(grad, resid, kblk, V, rotate=seed, step=t)   # resid updated in place

Both roundings may be stochastic instead (include/ina_i8_sr.h; ByteWireAggregator(rounding="stochastic")): the
stateless alternative to the residual, and the only one that reaches the owner's second rounding.  The rounding
stream (seed, step, sub, e0) is apart from the rotation's (rotate, step, rot_sub, rot_e0): ranks share the
second and must differ in the first.  tests/_i8_sr_ref.py replays the contract.

    kblk = i8.block_scales_sr([grad], V, rotate=seed, step=t)       # one quantum of headroom; then MIN
    q8, flags = i8.quantize_sr(grad, kblk, V, seed, rotate=seed, step=t, sub=1 + rank)
    q8s, sh = i8.sum_slices_requant_sr(received, V, seed, step=t, sub=65, e0=rank * shard)

`rotate` is None (no rotation) or the seed.  n must be a multiple of V for the block calls, buffers 16-byte
aligned, e0 a multiple of 128 and of V; no base; no CPU fallback and no value-by-value path.
"""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import MAX_WORKERS, check, load
from .ops import _blk_scales_arg, _fits, _grad_bufs, _ptrs, _req, _req_grad, _same_device, _stream
from .rot import _key, _v
from .sr import _params


def scale_for(absmax: float) -> int:
    """The largest k in [-126, 127] with absmax * 2^k + 1/2 <= 127, whatever the number of ranks: the sum's
    headroom is the int16 accumulator's."""
    k = C.c_int(0)
    check(load().ina_scale_for_i8(float(absmax), C.byref(k)), "i8.scale_for")
    return k.value


def _sr(rotate, step, sub, e0, V):
    """The ina_sr_t of a rotated call, or None (a NULL sr) for rotate=None."""
    return None if rotate is None else C.byref(_key(rotate, step, sub, e0, V))


def block_scales(xs, V: int, rotate: int | None = None, step: int = 0, sub: int = 0, e0: int = 0,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """int8 [n / V]: for each block scale_for(max |r|) over the given buckets, r the rotated values under
    `rotate`.  Ranks of one job agree on a block's scale by taking the MIN of theirs."""
    xs, n, xt = _grad_bufs(xs, "xs")
    V = _v(V, n)
    prm = _sr(rotate, step, sub, e0, V)
    out = _blk_scales_arg(out, n // V, xs[0], "out")
    check(load().ina_block_scales_i8(_ptrs(xs), xt, len(xs), n, V, out.data_ptr(), prm, _stream(xs[0])),
          "i8.block_scales")
    return out


def quantize(x: torch.Tensor, kblk: torch.Tensor, V: int, rotate: int | None = None, step: int = 0, sub: int = 0,
             e0: int = 0, out: torch.Tensor | None = None, overflow: torch.Tensor | None = None):
    """(int8 [n], flags): clamp(rne(r * 2^kblk[block]), -127, 127), NaN -> 0; one rank-local flag per block,
    1 where a value clamped or was NaN."""
    xt = _req_grad(x, "x")
    n = x.numel()
    V = _v(V, n)
    prm = _sr(rotate, step, sub, e0, V)
    kblk = _blk_scales_arg(kblk, n // V, x, given=True)
    out = torch.empty(n, dtype=torch.int8, device=x.device) if out is None else out
    _fits(out, n)
    _req(out, torch.int8, "out")
    overflow = torch.empty(n // V, dtype=torch.uint8, device=x.device) if overflow is None else overflow
    _fits(overflow, n // V, "overflow")
    _req(overflow, torch.uint8, "overflow")
    _same_device(x, out, overflow)
    check(load().ina_quantize_i8_wire(x.data_ptr(), xt, kblk.data_ptr(), V, out.data_ptr(), n, overflow.data_ptr(),
                                      prm, _stream(x)), "i8.quantize")
    return out, overflow


def scale_for_sr(absmax: float) -> int:
    """The largest k in [-126, 127] with absmax * 2^k + 1 <= 127: scale_for with the whole quantum of headroom
    that rounding up by chance needs."""
    k = C.c_int(0)
    check(load().ina_scale_for_i8_sr(float(absmax), C.byref(k)), "i8.scale_for_sr")
    return k.value


def block_scales_sr(xs, V: int, rotate: int | None = None, step: int = 0, sub: int = 0, e0: int = 0,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """block_scales under scale_for_sr's rule: the scales quantize_sr never clamps under.  (rotate, step, sub, e0)
    is the rotation's key; no random stream of the rounding takes part."""
    xs, n, xt = _grad_bufs(xs, "xs")
    V = _v(V, n)
    prm = _sr(rotate, step, sub, e0, V)
    out = _blk_scales_arg(out, n // V, xs[0], "out")
    check(load().ina_block_scales_i8_sr(_ptrs(xs), xt, len(xs), n, V, out.data_ptr(), prm, _stream(xs[0])),
          "i8.block_scales_sr")
    return out


def quantize_sr(x: torch.Tensor, kblk: torch.Tensor, V: int, seed: int, rotate: int | None = None, step: int = 0,
                sub: int = 0, e0: int = 0, rot_sub: int = 0, rot_e0: int = 0, out: torch.Tensor | None = None,
                overflow: torch.Tensor | None = None):
    """(int8 [n], flags): quantize with the rounding replaced by y = floor(t) + (u < t - floor(t)), t = r *
    2^kblk[block], u 24 bits of Philox under the rounding key (seed, step, sub, e0) -- e0 a multiple of 4.  The
    rotation's key is (rotate, step, rot_sub, rot_e0).  E[q8] = t where nothing clamps."""
    xt = _req_grad(x, "x")
    n = x.numel()
    V = _v(V, n)
    prm = _sr(rotate, step, rot_sub, rot_e0, V)
    rnd = _params(seed, step, sub, e0)
    kblk = _blk_scales_arg(kblk, n // V, x, given=True)
    out = torch.empty(n, dtype=torch.int8, device=x.device) if out is None else out
    _fits(out, n)
    _req(out, torch.int8, "out")
    overflow = torch.empty(n // V, dtype=torch.uint8, device=x.device) if overflow is None else overflow
    _fits(overflow, n // V, "overflow")
    _req(overflow, torch.uint8, "overflow")
    _same_device(x, out, overflow)
    check(load().ina_quantize_sr_i8_wire(x.data_ptr(), xt, kblk.data_ptr(), V, out.data_ptr(), n, overflow.data_ptr(),
                                         prm, C.byref(rnd), _stream(x)), "i8.quantize_sr")
    return out, overflow


def _resid(resid, x: torch.Tensor, name: str = "resid"):
    """A rank-local residual: float32 whatever x's dtype, one value per value of x, on x's device."""
    _req(resid, torch.float32, name)
    if resid.numel() != x.numel():
        raise ValueError(f"{name} holds {resid.numel()} elements, the bucket {x.numel()}")
    _same_device(x, resid)


def block_scales_ef(xs, resids, V: int, rotate: int | None = None, step: int = 0, sub: int = 0, e0: int = 0,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """block_scales over xs[w] + resids[w] (include/ina_i8_ef.h): the scales of what quantize_ef will quantise.
    Nothing but the scales is written; ranks agree by taking the MIN of theirs."""
    xs, n, xt = _grad_bufs(xs, "xs")
    resids = [resids] if isinstance(resids, torch.Tensor) and resids.dim() == 1 else list(resids)
    if len(resids) != len(xs):
        raise ValueError("one residual per bucket")
    for i, r in enumerate(resids):
        _resid(r, xs[0], f"resids[{i}]")
    V = _v(V, n)
    prm = _sr(rotate, step, sub, e0, V)
    out = _blk_scales_arg(out, n // V, xs[0], "out")
    check(load().ina_block_scales_i8_ef(_ptrs(xs), _ptrs(resids), xt, len(xs), n, V, out.data_ptr(), prm,
                                        _stream(xs[0])), "i8.block_scales_ef")
    return out


def quantize_ef(x: torch.Tensor, resid: torch.Tensor, kblk: torch.Tensor, V: int, rotate: int | None = None,
                step: int = 0, sub: int = 0, e0: int = 0, out: torch.Tensor | None = None,
                overflow: torch.Tensor | None = None):
    """(int8 [n], flags): quantize of x + resid, in one launch with resid's update in place: resid becomes the
    rounding error r - q8 * 2^-kblk[block] taken back through the inverse rotation (as it is under rotate=None),
    +0 where that is NaN or inf.  resid must not overlap x or out."""
    xt = _req_grad(x, "x")
    n = x.numel()
    _resid(resid, x)
    V = _v(V, n)
    prm = _sr(rotate, step, sub, e0, V)
    kblk = _blk_scales_arg(kblk, n // V, x, given=True)
    out = torch.empty(n, dtype=torch.int8, device=x.device) if out is None else out
    _fits(out, n)
    _req(out, torch.int8, "out")
    overflow = torch.empty(n // V, dtype=torch.uint8, device=x.device) if overflow is None else overflow
    _fits(overflow, n // V, "overflow")
    _req(overflow, torch.uint8, "overflow")
    _same_device(x, out, overflow)
    check(load().ina_quantize_ef_i8_wire(x.data_ptr(), xt, resid.data_ptr(), kblk.data_ptr(), V, out.data_ptr(), n,
                                         overflow.data_ptr(), prm, _stream(x)), "i8.quantize_ef")
    return out, overflow


def _slices(parts):
    """The 1..64 int8 slices of a sum, of one length: (list, n)."""
    parts = list(parts.unbind(0)) if isinstance(parts, torch.Tensor) and parts.dim() > 1 else list(parts)
    if not 1 <= len(parts) <= MAX_WORKERS:
        raise ValueError(f"1..{MAX_WORKERS} slices, got {len(parts)}")
    for p in parts:
        _req(p, torch.int8, "parts")
    n = parts[0].numel()
    if any(p.numel() != n for p in parts):
        raise ValueError("every slice must hold the same number of values")
    return parts, n


def sum_slices(parts, out: torch.Tensor | None = None) -> torch.Tensor:
    """int16 [n]: the exact element-wise sum of 1..64 int8 slices of n values each (any n)."""
    parts, n = _slices(parts)
    out = torch.empty(n, dtype=torch.int16, device=parts[0].device) if out is None else out
    _fits(out, n)
    _req(out, torch.int16, "out")
    _same_device(out, *parts)
    check(load().ina_sum_i8_slices(_ptrs(parts), len(parts), out.data_ptr(), n, _stream(out)), "i8.sum_slices")
    return out


def sum_slices_requant(parts, V: int, out: torch.Tensor | None = None, shift: torch.Tensor | None = None):
    """(int8 [n], uint8 [n / V]): the exact sum of 1..64 int8 slices, each block of V sums rounded to nearest
    even under the block's shift -- the smallest in [0, 7] that brings its largest |sum| to at most 127 -- in
    one launch (include/ina_i8_gather.h).  The sum is about q8 * 2^shift; -128 is never written."""
    parts, n = _slices(parts)
    V = _v(V, n)
    out = torch.empty(n, dtype=torch.int8, device=parts[0].device) if out is None else out
    _fits(out, n)
    _req(out, torch.int8, "out")
    shift = torch.empty(n // V, dtype=torch.uint8, device=out.device) if shift is None else shift
    _fits(shift, n // V, "shift")
    _req(shift, torch.uint8, "shift")
    _same_device(out, shift, *parts)
    check(load().ina_sum_i8_slices_requant(_ptrs(parts), len(parts), V, out.data_ptr(), shift.data_ptr(), n,
                                           _stream(out)), "i8.sum_slices_requant")
    return out, shift


def sum_slices_requant_sr(parts, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0,
                          out: torch.Tensor | None = None, shift: torch.Tensor | None = None):
    """(int8 [n], uint8 [n / V]): sum_slices_requant with q8 = (S + u) >> shift, u the low `shift` bits of a
    Philox byte under (seed, step, sub, e0) -- e0 a multiple of 16 -- and shift the smallest with max |S| <=
    127 << shift.  Integers only: E[q8] * 2^shift = S exactly; a block within +-127 is sum_slices_requant's."""
    rnd = _params(seed, step, sub, e0)
    if e0 % 16:
        raise ValueError(f"e0 must be a multiple of 16, got {e0}: a lane's 16 values share one Philox call")
    parts, n = _slices(parts)
    V = _v(V, n)
    out = torch.empty(n, dtype=torch.int8, device=parts[0].device) if out is None else out
    _fits(out, n)
    _req(out, torch.int8, "out")
    shift = torch.empty(n // V, dtype=torch.uint8, device=out.device) if shift is None else shift
    _fits(shift, n // V, "shift")
    _req(shift, torch.uint8, "shift")
    _same_device(out, shift, *parts)
    check(load().ina_sum_i8_slices_requant_sr(_ptrs(parts), len(parts), V, out.data_ptr(), shift.data_ptr(), n,
                                              C.byref(rnd), _stream(out)), "i8.sum_slices_requant_sr")
    return out, shift


def dequantize_gather(q8: torch.Tensor, shift: torch.Tensor, kblk: torch.Tensor, V: int, rotate: int | None = None,
                      step: int = 0, sub: int = 0, e0: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """float32: bit for bit rot.dequantize (rotate=seed) or blk.dequantize (rotate=None) of the int16 values
    q8 << shift[block], read from the bytes.  A shift above 7 is read as 7."""
    _req(q8, torch.int8, "q8")
    n = q8.numel()
    V = _v(V, n)
    prm = _sr(rotate, step, sub, e0, V)
    _req(shift, torch.uint8, "shift")
    _fits(shift, n // V, "shift")
    kblk = _blk_scales_arg(kblk, n // V, q8, given=True)
    out = torch.empty(q8.shape, dtype=torch.float32, device=q8.device) if out is None else out
    _fits(out, n)
    _req(out, torch.float32, "out")
    _same_device(q8, shift, out)
    check(load().ina_dequantize_i8_gather(q8.data_ptr(), shift.data_ptr(), kblk.data_ptr(), V, out.data_ptr(), n,
                                          prm, _stream(q8)), "i8.dequantize_gather")
    return out
